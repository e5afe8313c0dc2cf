"""The per-edge layer reference (tests/layer_ref.py) checked on the CPU: by hand, against the oracle the golden fixtures pin, against
torch autograd, and its own fp32 evaluation against the bound the GPU tests use (so the bound is known to be satisfiable by a correct
fp32 implementation before a GPU is involved)."""
import math

import numpy as np
import pytest
import torch

from oracle import redgnn_oracle as orc
from tests import layer_ref as lr


def test_layer_ref_on_five_edges_by_hand():
    """One query, two old nodes, two new nodes, two relations, d = 1, attn_dim = 1 (ap = 4), w = 1, b_alpha = 0:

        hidden = [1, 2]   rela = [10, 20]   a_s = [ln 3, -1]   a_r = a_q = 0   grad_agg G = [1, 2]
        edge  s r o   z = relu(a_s[s])   alpha            m = hidden[s] + rela[r]   g_alpha = G[o] m   g_p = g_alpha alpha (1 - alpha)
        e0    0 0 0   ln 3               3/4              11                        11                 2.0625
        e1    0 1 1   ln 3               3/4              21                        42                 7.875
        e2    1 0 0   0                  1/2              12                        12                 3
        e3    1 1 1   0                  1/2              22                        44                 11
        e4    1 1 1   0                  1/2              22  (the same fact twice) 44                 11

        agg         = [3/4 11 + 1/2 12, 3/4 21 + 1/2 22 + 1/2 22]            = [14.25, 37.75]
        grad_hidden = [3/4 1 + 3/4 2, 1/2 1 + 1/2 2 + 1/2 2]                 = [2.25, 2.5]
        grad_rela   = [3/4 1 + 1/2 1, 3/4 2 + 1/2 2 + 1/2 2]                 = [1.25, 3.5]
        g_z = g_p w 1[z > 0]: e0 2.0625, e1 7.875, the others 0 (relu is off)
        grad_a_s = [9.9375, 0]   grad_a_r = [2.0625, 7.875]   grad_a_q = [9.9375]
        grad_w_alpha = (2.0625 + 7.875) ln 3      grad_b_alpha = 2.0625 + 7.875 + 3 + 11 + 11 = 34.9375
        S(agg[0]) = kappa_0 |m_0| + kappa_2 |m_2| with kappa = alpha + alpha (1 - alpha) Z:  Z_0 = ln 3, Z_2 = |-1| = 1
                  = (3/4 + 3/16 ln 3) 11 + (1/2 + 1/4) 12
    """
    ln3 = math.log(3.0)
    edges = np.array([[0, 7, 0, 8, 0, 0], [0, 7, 1, 9, 0, 1], [0, 5, 0, 8, 1, 0], [0, 5, 1, 9, 1, 1], [0, 5, 1, 9, 1, 1]])
    hop = lr.static_hop(edges, 2, 2)
    pad = lambda col: np.concatenate([np.asarray(col, np.float64).reshape(-1, 1), np.zeros((len(col), 3))], 1)
    args = (hop, np.array([[1.0], [2.0]]), np.array([[10.0], [20.0]]), None, pad([ln3, -1.0]), pad([0.0, 0.0]), pad([0.0]),
            np.array([1.0]), np.array([0.0]))
    f = lr.forward(*args)
    np.testing.assert_allclose(f.alpha, [0.75, 0.75, 0.5, 0.5, 0.5], rtol=1e-15)
    np.testing.assert_allclose(f.agg[:, 0], [14.25, 37.75], rtol=1e-15)
    np.testing.assert_allclose(f.S["agg"][0, 0], (0.75 + 0.1875 * ln3) * 11 + 0.75 * 12, rtol=1e-15)
    assert f.n["agg"][:, 0].tolist() == [2, 3]
    b = lr.backward(*args, np.array([[1.0], [2.0]]))
    np.testing.assert_allclose(b.grad_hidden[:, 0], [2.25, 2.5], rtol=1e-15)
    np.testing.assert_allclose(b.grad_rela[:, 0], [1.25, 3.5], rtol=1e-15)
    np.testing.assert_allclose(b.grad_a_s, pad([9.9375, 0.0]), rtol=1e-14)
    np.testing.assert_allclose(b.grad_a_r, pad([2.0625, 7.875]), rtol=1e-14)
    np.testing.assert_allclose(b.grad_a_q, pad([9.9375]), rtol=1e-14)
    np.testing.assert_allclose(b.grad_w_alpha, [9.9375 * ln3], rtol=1e-14)
    np.testing.assert_allclose(b.grad_b_alpha, [34.9375], rtol=1e-14)
    assert b.grad_time is None and b.n["grad_a_s"][:, 0].tolist() == [2, 3] and b.n["grad_b_alpha"] == 5


def test_forward_equals_the_oracle_layer():
    """forward == orc.gnn_layer_forward's agg and alpha in fp64 when the hoisted tables are formed from the same state dict."""
    rng = np.random.default_rng(3)
    n_ent, n_rel, d, attn, B = 60, 4, 24, 5, 7
    trip = np.stack([rng.integers(0, n_ent, 400), rng.integers(0, n_rel, 400), rng.integers(0, n_ent, 400)], 1)
    og = orc.OracleGraph(orc.double_triple(trip, n_rel), n_ent, n_rel)
    nodes0 = np.stack([np.arange(B), rng.integers(0, n_ent, B)], 1)
    nodes1, _, _ = orc.get_neighbors(og, nodes0)
    nodes2, edges, _ = orc.get_neighbors(og, nodes1)
    q_rel = rng.integers(0, 2 * n_rel, B)
    p = {"l.rela_embed.weight": rng.standard_normal((2 * n_rel + 1, d)), "l.Ws_attn.weight": rng.standard_normal((attn, d)),
         "l.Wr_attn.weight": rng.standard_normal((attn, d)), "l.Wqr_attn.weight": rng.standard_normal((attn, d)),
         "l.Wqr_attn.bias": rng.standard_normal(attn), "l.w_alpha.weight": rng.standard_normal((1, attn)),
         "l.w_alpha.bias": rng.standard_normal(1), "l.W_h.weight": rng.standard_normal((d, d))}
    hidden = rng.standard_normal((len(nodes1), d))
    _, agg, alpha = orc.gnn_layer_forward(p, "l.", q_rel, torch.as_tensor(hidden), edges, len(nodes2), torch.relu, dtype=torch.float64)
    rela = p["l.rela_embed.weight"]
    ap = 8
    pad = lambda x: np.concatenate([x, np.zeros((len(x), ap - attn))], 1)
    f = lr.forward(lr.static_hop(edges, len(nodes1), len(nodes2)), hidden, rela, None, pad(hidden @ p["l.Ws_attn.weight"].T),
                   pad(rela @ p["l.Wr_attn.weight"].T), pad(rela[q_rel] @ p["l.Wqr_attn.weight"].T + p["l.Wqr_attn.bias"]),
                   p["l.w_alpha.weight"][0], p["l.w_alpha.bias"])
    np.testing.assert_allclose(f.agg, agg.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.alpha, alpha.numpy()[:, 0], rtol=1e-12, atol=1e-12)


def _torch_forward(hop, hidden, rela, time_tab, a_s, a_r, a_q, w, b):
    """The forward in ten lines of torch, for autograd."""
    ix = lambda a: torch.as_tensor(a, dtype=torch.long)
    wp = torch.cat([w, torch.zeros(a_s.shape[1] - len(w), dtype=w.dtype)])
    z = torch.relu(a_s[ix(hop.s)] + a_r[ix(hop.r)] + a_q[ix(hop.b)])
    alpha = torch.sigmoid(z @ wp + b[0])
    m = hidden[ix(hop.hrow)] + rela[ix(hop.rrow)]
    if hop.trow is not None:
        m = m + time_tab[ix(hop.trow)]
    return torch.zeros(hop.n_new, hidden.shape[1], dtype=hidden.dtype).index_add_(0, ix(hop.o), alpha[:, None] * m)


@pytest.mark.parametrize("name", ["b31_e97", "temporal", "windowed"])
def test_backward_equals_autograd(name):
    """backward == torch autograd (fp64) through _torch_forward, all outputs, static / temporal / windowed."""
    case = lr.CASES[name]()
    for k, (_, _, _, hop) in enumerate(lr.hops(case)):
        x = lr.inputs(case, k, hop)
        keys = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")
        t = [None if x[n] is None else torch.tensor(x[n], dtype=torch.float64, requires_grad=True) for n in keys]
        agg = _torch_forward(hop, *t)
        agg.backward(torch.as_tensor(x["grad_agg"], dtype=torch.float64))
        b = lr.backward(hop, *(x[n] for n in keys), x["grad_agg"])
        np.testing.assert_allclose(lr.forward(hop, *(x[n] for n in keys)).agg, agg.detach().numpy(), rtol=1e-12, atol=1e-12)
        for out, ten in zip(("grad_hidden", "grad_rela", "grad_time", "grad_a_s", "grad_a_r", "grad_a_q", "grad_w_alpha", "grad_b_alpha"), t):
            if ten is None:
                assert getattr(b, out) is None
                continue
            g = ten.grad.numpy() if ten.grad is not None else np.zeros(ten.shape)
            np.testing.assert_allclose(getattr(b, out), g, rtol=1e-10, atol=1e-10, err_msg="%s hop %d %s" % (name, k + 1, out))


def test_table_covers_what_it_names():
    """The cases reach the regimes their names promise (checked on the oracle's edge lists, no GPU)."""
    t = lr.hops(lr.CASES["temporal"]())[1][3]
    assert set(np.unique(t.dir)) == {0, 1, 2} and np.abs(t.dt).max() == 11
    c = lr.CASES["windowed"]()
    hs = lr.hops(c)
    w = hs[1][3]
    assert w.trow.min() == 0 and w.trow.max() == c.n_tab - 1
    first = hs[0][2]
    for q in (0, 2, 3):      # empty window, older than the first row, self-loop only: the identity edge alone
        assert (first[:, 0] == q).sum() == 1
    c = lr.CASES["hubs"]()
    e = lr.hops(c)[0][2]
    q0 = e[e[:, 0] == 0]
    assert sorted(np.bincount(q0[:, 3])[:7].tolist()) == sorted(np.bincount(q0[:, 1])[:7].tolist()) == [1, 127, 128, 129, 256, 257, 3000]
    for name in ("wide_ent_ld64", "t_wide_ent_ld64", "ent_2p20"):
        c = lr.CASES[name]()
        e = np.concatenate([h[2] for h in lr.hops(c)], 0)
        assert (e[:, 1] == c.n_ent - 1).any() and (e[:, 3] == c.n_ent - 1).any() and ((e[:, 1] == c.n_ent - 1) & (e[:, 3] != c.n_ent - 1)).any()
    for name in ("wide_rel_ld64", "rel_4095"):
        c = lr.CASES[name]()
        e = np.concatenate([h[2] for h in lr.hops(c)], 0)
        assert c.n_rela_rows in (4101, 4095) and (e[:, 2] == c.n_rela_rows - 1).any() and (e[:, 2] >= c.n_rel).any()
    for name in ("tickets", "tickets_d48"):
        c = lr.CASES[name]()
        og = lr.oracle_graph(c)
        (_, _, _, h), = lr.hops(c)
        indeg = np.bincount(og.KG[:, 2], minlength=c.n_ent)
        bw, packs = (c.B + 31) // 32, -(-len(og.KG) // 128)      # (at least: a pack holds whole rows or segments, 128 entries at most)
        assert (len(og.KG), bw, h.n_new, h.E) == (40514, 32, 65931, 82760) and c.d == (64 if name == "tickets" else 48) == c.ld
        assert sorted(indeg[indeg > 128].tolist()) == [2069, 2075]      # two cut rows: partial sums and their `written` bytes
        # items per ticket the work space allows (layer_fwd.hip wp_tickets: n_items / 8192, at most 32), walks 2 .. 7
        assert [min(bw * (1 << (w - 2)) * packs // 8192, 32) for w in range(2, 8)] == [1, 2, 4, 9, 19, 32]
        assert c.B * ((c.n_ent + 31) // 32) == 16384 > 12288      # frontier.hip SMALL_MAX_WORDS
    s = lr.CASES["saturated"]()
    h = lr.hops(s)[1][3]
    x = lr.inputs(s, 1, h)
    a = lr.forward(h, x["hidden"], x["rela"], None, x["a_s"], x["a_r"], x["a_q"], x["w_alpha"], x["b_alpha"]).alpha
    assert np.mean(np.minimum(a, 1 - a) < 1e-6) > 0.5
    dd = lr.CASES["dead"]()
    h = lr.hops(dd)[0][3]
    x = lr.inputs(dd, 0, h)
    keys = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")
    b = lr.backward(h, *(x[n] for n in keys), x["grad_agg"])
    assert not b.grad_a_s.any() and not b.grad_w_alpha.any() and b.grad_b_alpha[0] != 0


@pytest.mark.parametrize("name", list(lr.CASES))
def test_fp32_reference_within_its_bound(name):
    """The reference evaluated in np.float32 (same code, same edge order) against its fp64 self on every case of the table: the ratio
    |ref32 - ref64| / ((n + n0) u S) stays below REF32_WORST_RATIO for every element of every output, i.e. the GPU's bound (C_BOUND =
    4 x that) is one a correct fp32 implementation meets with a factor 4 to spare.  Prints the ratios."""
    case = lr.CASES[name]()
    keys = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")
    for k, (_, _, _, hop) in enumerate(lr.hops(case)):
        x = lr.inputs(case, k, hop)
        a = [hop] + [x[n] for n in keys]
        f64, f32 = lr.forward(*a), lr.forward(*a, dtype=np.float32)
        b64, b32 = lr.backward(*a, x["grad_agg"]), lr.backward(*a, x["grad_agg"], dtype=np.float32)
        assert f32.agg.dtype == np.float32 and b32.grad_a_s.dtype == np.float32
        ratios = {"agg": lr.worst_ratio(f32.agg, f64.agg, f64.S["agg"], f64.n["agg"], lr.n0_of("agg", case.d, case.attn_dim))}
        for o in lr.BWD_OUTPUTS:
            if getattr(b64, o) is not None:
                ratios[o] = lr.worst_ratio(getattr(b32, o), getattr(b64, o), b64.S[o], b64.n[o], lr.n0_of(o, case.d, case.attn_dim))
        print("%s hop %d (n_old %d, n_new %d, E %d): %s" % (name, k + 1, hop.n_old, hop.n_new, hop.E,
                                                           " ".join("%s=%.3g" % kv for kv in ratios.items())))
        for o, r in ratios.items():
            assert r <= lr.REF32_WORST_RATIO, (name, k + 1, o, r)
