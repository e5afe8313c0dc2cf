"""Reference and case table of the hop kernels called on their own: csrc/explain.hip (rg_explain_seed / _count / _emit / _gather and
the rg_texplain_* / rg_xexplain_* instantiations) and csrc/profile.hip (rg_attn_profile, rg_tattn_profile, rg_xattn_profile).  Plain
numpy, no GPU.  TEST INFRASTRUCTURE.

The cases are tests/layer_ref.py's (a subset of its table, built by its constructors; nothing is added to layer_ref.CASES) plus, in a
table of this module's own:

  gw8 / gw16 / gw32 / gw64   profile.hip profile_hop picks the words per wave step as
                                 gw = 64; while (gw > 4 && batch * ceil(W / gw) < 8192) gw >>= 1
                             B = 1024 with n_ent = 2060 / 4100 / 8200 / 16400 (W = 65 / 129 / 257 / 513) gives 8 / 16 / 32 / 64 (``gw_of``
                             restates the formula).  Three queries start from a random 40 % of the entities, so that a wave step lists
                             more than 64 heads (the k0 loop iterates, node id = s_base + k0 + sl) whose out-edges number more than 64
                             (the x0 loop iterates); ``dense_steps`` counts such steps from the oracle's node list.
  x_lds80                    a windowed case whose extrapolation profile takes the LDS path between 64 KiB and 80 KiB (the launch that
                             raises hipFuncAttributeMaxDynamicSharedMemorySize): 463 relation rows, ap = 8, 8 lag bins (``xlds_bytes``).

What is compared with what:

  expected_hop_edges   the hop-l edges into a set of marked tails, from the graph's CSR by tail and the level-(l-1) node list, in the
                       kernel's output order (row, tail, CSR position), with the heads' bitmap: explain.hip's contract restated densely
  expected_profile     per (query, [direction | lag bin,] relation) the number of edges and the sum of rint(alpha_f32 * 2^32) as int64.
                       The scaling by a power of two is exact and np.rint rounds half to even as llrintf does, so this is the kernel's
                       integer, not an approximation of it
  one-hot readout      with hidden = 0, time table = 0 and rela[row of r, r % d] = 1 the layer forward writes agg[o, r % d] = alpha_e
                       for every edge that is alone in its (new node, r % d) group (m = 1.0 exactly, a sum of one term; the other edges
                       into o add alpha * 0.0): the forward's alpha can be read bit for bit.  ``singleton_mask`` names those edges
  alpha_bound          |alpha_fp32 - alpha_fp64| <= C_BOUND * (1 + n0) * u * kappa + tiny: layer_ref's agg bound for one term with |m| = 1
"""
import types

import numpy as np

from tests import layer_ref as lr

KEYS = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")
SCALE = 2.0 ** 32
Q = 2.0 ** -33                     # the rounding of one alpha to the profile's fixed point

# ---- the case table ---------------------------------------------------------------------------------------------------------------------
FROM_LAYER_REF = (
    "default", "ap_1", "ap_3", "ap_4", "ap_12", "ap_16", "ap_17", "ap_32",      # every with_ap4 instance
    "hubs",                                                                      # in-degree 3000: cnt carries across 64-edge chunks
    "short_rows_dense",
    "b1_e33", "b31_e97", "b65_e97", "b33_e1000",
    "tickets",                                                                   # B = 1024, 16384 bitmap words
    "wide_ent_ld64", "t_wide_ent_ld64",                                          # W = 32770
    "wide_rel_ld64", "t_wide_rel_ld64",                                          # 4101 relation rows: the profile's global-bin path
    "temporal", "windowed", "saturated", "dead",
)
GW_CASES = {"gw8": 2060, "gw16": 4100, "gw32": 8200, "gw64": 16400}
N_DENSE = 3                        # queries of a gw case that start from a dense node set
XLDS = "x_lds80"
XLDS_BINS = 8


def gw_of(batch, n_ent):
    """profile.hip profile_hop: words of the level bitmap per wave step."""
    W = (n_ent + 31) // 32
    gw = 64
    while gw > 4 and batch * -(-W // gw) < 8192:
        gw >>= 1
    return gw


def _gw_case(name, n_ent, seed):
    rng = np.random.default_rng(seed)
    B = 1024
    dense = lr._dense_start(rng, N_DENSE, n_ent, 0.4)
    rest = lr._subjects(rng, B - N_DENSE, n_ent)
    rest[:, 0] += N_DENSE
    return lr._case(name, seed=seed, n_ent=n_ent, n_rel=5, m=3000, B=B, hops=1, nodes0=np.concatenate([dense, rest], 0))


def xlds_bytes(n_rela_rows, ap, n_bins, n_lag):
    """profile.hip, LAG mode: the 16 KiB head list, per relation row the a_r row and n_bins cells of 8 + 4 bytes, the lag table."""
    return 16384 + n_rela_rows * (4 * ap + 12 * n_bins) + n_lag


CASES = {name: lr.CASES[name] for name in FROM_LAYER_REF}
CASES.update({name: (lambda name=name, n_ent=n_ent, i=i: _gw_case(name, n_ent, 50 + i)) for i, (name, n_ent) in enumerate(GW_CASES.items())})
# ICEWS14-like: 2 * 231 + 1 = 463 relation rows, attn_dim 5 (ap = 8), a time table of 8 rows binned by the identity
CASES[XLDS] = lambda: lr._windowed_case(XLDS, seed=56, n_rel=231, n_tab=XLDS_BINS)
# cases small enough for the B = 1 re-run of single rows
SMALL = ("default", "ap_3", "b1_e33", "b31_e97", "b65_e97", "temporal", "windowed", "saturated")


def dense_steps(case, nodes_old, out_deg):
    """Over the wave steps (gw words of one query's level bitmap) of a hop: (the largest number of heads in a step, the largest number
    of out-edges of 64 consecutive heads of a step that lists more than 64).  Both above 64: profile.hip's k0 and x0 loops iterate."""
    gw = gw_of(case.B, case.n_ent)
    nodes_old = np.asarray(nodes_old, np.int64)
    step = nodes_old[:, 0] * (1 << 32) + nodes_old[:, 1] // (32 * gw)
    uniq, first, n_heads = np.unique(step, return_index=True, return_counts=True)
    most = 0
    for f, n in zip(first[n_heads > 64], n_heads[n_heads > 64]):
        deg = out_deg[nodes_old[f:f + n, 1]]
        most = max(most, max(int(deg[k0:k0 + 64].sum()) for k0 in range(0, n, 64)))
    return int(n_heads.max(initial=0)), most


# ---- bitmaps ----------------------------------------------------------------------------------------------------------------------------
def n_words(n_ent):
    return (n_ent + 31) // 32


def bitmap(nodes, B, n_ent):
    """uint32 [B, W] with one bit per (row, entity) of ``nodes`` (the frontier's batch-major word layout)."""
    nodes = np.asarray(nodes, np.int64).reshape(-1, 2)
    assert len(nodes) == 0 or (nodes.min() >= 0 and nodes[:, 0].max() < B and nodes[:, 1].max() < n_ent)
    m = np.zeros((B, n_words(n_ent)), np.uint32)
    np.bitwise_or.at(m, (nodes[:, 0], nodes[:, 1] >> 5), np.uint32(1) << (nodes[:, 1] & 31).astype(np.uint32))
    return m


def bitmap_nodes(marks):
    """int64 [n, 2] (row, entity) of the set bits, sorted."""
    marks = np.ascontiguousarray(marks, np.uint32)
    B, W = marks.shape
    bits = np.flatnonzero(np.unpackbits(marks.view(np.uint8).reshape(-1), bitorder="little"))
    return np.stack([bits // (32 * W), bits % (32 * W)], 1).astype(np.int64)


# ---- the graph by tail --------------------------------------------------------------------------------------------------------------------
def csr_by_tail(og):
    """(in_ptr, in_head_rel [n_fact, 2], in_time [n_fact] or None) of an oracle graph: its rows in a stable order by tail.  For CPU tests;
    the GPU tests take the library's own arrays (Graph.export / export_time), whose order inside a tail's row is the library's."""
    KG = np.asarray(og.KG, np.int64)
    order = np.argsort(KG[:, 2], kind="stable")
    ptr = np.zeros(og.n_ent + 1, np.int64)
    np.add.at(ptr, KG[:, 2] + 1, 1)
    return np.cumsum(ptr), KG[order][:, :2], (KG[order, 3] if KG.shape[1] > 3 else None)


class AlphaTable:
    """alpha as a function of (row, head, relation) - what the attention reads - from one listing of a hop's edges."""

    def __init__(self, n_ent, n_rela_rows, b, head, rel, alpha):
        self.n_ent, self.R = int(n_ent), int(n_rela_rows)
        key = self._key(b, head, rel)
        alpha = np.asarray(alpha)
        self.keys, first, inv = np.unique(key, return_index=True, return_inverse=True)
        self.vals = alpha[first]
        same = self.vals[inv] == alpha
        assert same.all(), "alpha differs between two edges with the same (row, head, relation): %d edges" % int((~same).sum())

    def _key(self, b, head, rel):
        return (np.asarray(b, np.int64) * self.n_ent + np.asarray(head, np.int64)) * self.R + np.asarray(rel, np.int64)

    def at(self, b, head, rel):
        key = self._key(b, head, rel)
        i = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1) if len(self.keys) else np.zeros(len(key), np.int64)
        assert len(key) == 0 or (len(self.keys) and (self.keys[i] == key).all()), "an edge the table has no alpha for"
        return self.vals[i] if len(key) else self.vals[:0]


def hop_candidates(case, graph_export, nodes_old, marks):
    """The in-edges of the marked tails that the hop has whatever their alpha: for every set bit (b, t) of ``marks`` (uint32 [B, W]) the
    in-edges of t in the order of ``graph_export`` = (in_ptr, in_head_rel, in_time or None) whose head is in ``nodes_old`` (level l-1,
    int64 [n, 2] sorted) for row b and whose data row (windowed cases: in_time) is a self-loop or inside [win_lo[b], win_hi[b]).  In (row,
    tail, CSR position) order."""
    in_ptr, in_hr, in_time = graph_export
    in_ptr = np.asarray(in_ptr, np.int64)
    in_hr = np.asarray(in_hr, np.int64)
    nodes_old = np.asarray(nodes_old, np.int64).reshape(-1, 2)
    B, W = case.B, n_words(case.n_ent)
    assert marks.shape == (B, W)
    bt = bitmap_nodes(marks)
    assert len(bt) == 0 or bt[:, 1].max() < case.n_ent, "a mark past the last entity"
    beg, deg = in_ptr[bt[:, 1]], in_ptr[bt[:, 1] + 1] - in_ptr[bt[:, 1]]
    which = np.repeat(np.arange(len(bt)), deg)
    pos = np.repeat(beg, deg) + np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
    b, t = bt[which, 0], bt[which, 1]
    head, rel = in_hr[pos, 0], in_hr[pos, 1]
    old_key = nodes_old[:, 0] * case.n_ent + nodes_old[:, 1]
    assert (np.diff(old_key) > 0).all()
    key = b * case.n_ent + head
    idx = np.minimum(np.searchsorted(old_key, key), max(len(old_key) - 1, 0))
    keep = old_key[idx] == key if len(old_key) else np.zeros(len(key), bool)
    if case.kind == "windowed":
        row = np.asarray(in_time, np.int64)[pos]
        keep &= (row >= case.n_data) | ((row >= np.asarray(case.win_lo, np.int64)[b]) & (row < np.asarray(case.win_hi, np.int64)[b]))
    b, t, head, rel, pos, idx = (x[keep] for x in (b, t, head, rel, pos, idx))
    return types.SimpleNamespace(b=b, t=t, head=head, rel=rel, pos=pos, old_idx=idx, B=B, W=W, n_ent=case.n_ent,
                                 time=None if in_time is None else np.asarray(in_time, np.int64)[pos])


def select_edges(c, alpha=None, tau=0.0):
    """The candidates whose alpha (an AlphaTable; None with tau <= 0: every edge passes) is >= tau.  Returns a namespace: edges int64
    [E, 4] = (row, head, rel, tail), pos (their CSR positions), old_idx (the heads' index in the level-(l-1) node list), time (in_time[pos]
    or None), alpha, heads (the heads' bitmap, uint32 [B, W]), word_count (kept edges per word of the marks, int64 [B * W])."""
    if alpha is None:
        assert tau <= 0
        al, k = None, slice(None)
    else:
        if getattr(c, "looked_up", None) is not alpha:      # (one look-up per candidate list and table, whatever the number of taus)
            c.looked_up, c.alpha = alpha, alpha.at(c.b, c.head, c.rel)
        al = c.alpha
        k = al >= tau
        al = al[k]
    b, t, head, rel = c.b[k], c.t[k], c.head[k], c.rel[k]
    return types.SimpleNamespace(edges=np.stack([b, head, rel, t], 1), pos=c.pos[k], old_idx=c.old_idx[k], alpha=al,
                                 time=None if c.time is None else c.time[k], heads=bitmap(np.stack([b, head], 1), c.B, c.n_ent),
                                 word_count=np.bincount(b * c.W + (t >> 5), minlength=c.B * c.W))


def expected_hop_edges(case, graph_export, nodes_old, marks, alpha=None, tau=0.0):
    """The hop's edges into the marked tails with alpha >= tau, in the kernel's output order: select_edges of hop_candidates."""
    return select_edges(hop_candidates(case, graph_export, nodes_old, marks), alpha, tau)


def brute_hop_edges(B, n_ent, in_ptr, in_hr, in_time, level_old, marked, alpha_of, tau, window=None):
    """expected_hop_edges as python loops over sets: level_old and marked are sets of (row, entity), alpha_of(b, head, rel) -> float,
    window = (win_lo, win_hi, n_data) or None.  Returns ([(row, head, rel, tail, pos)], set of (row, head))."""
    out, heads = [], set()
    for b in range(B):
        for t in range(n_ent):
            if (b, t) not in marked:
                continue
            for c in range(int(in_ptr[t]), int(in_ptr[t + 1])):
                h, r = int(in_hr[c][0]), int(in_hr[c][1])
                if (b, h) not in level_old:
                    continue
                if window is not None:
                    lo, hi, n_data = window
                    row = int(in_time[c])
                    if not (row >= n_data or lo[b] <= row < hi[b]):
                        continue
                if alpha_of(b, h, r) >= tau:
                    out.append((b, h, r, t, c))
                    heads.add((b, h))
    return out, heads


# ---- the profile --------------------------------------------------------------------------------------------------------------------------
def fixed_point(alpha_f32):
    """llrintf(alpha * 2^32) of float32 alphas, as int64."""
    a = np.asarray(alpha_f32)
    assert a.dtype == np.float32
    return np.rint(a.astype(np.float64) * SCALE).astype(np.int64)


def profile_cells(hop, B, n_rela_rows, kind="static", lag_bin=None, n_bins=None):
    """(shape of the profile's outputs, the flat cell of every edge of the hop in it; -1: the edge is dropped).  [B, R] (kind "static"),
    [B, 3, R] ("temporal": the edge's direction hop.dir) or [B, n_bins, R] ("windowed": bin = lag_bin[hop.trow], edges whose bin is
    >= n_bins dropped)."""
    b, r = np.asarray(hop.b, np.int64), np.asarray(hop.r, np.int64)
    if kind == "static":
        return (B, n_rela_rows), b * n_rela_rows + r
    if kind == "temporal":
        return (B, 3, n_rela_rows), (b * 3 + hop.dir) * n_rela_rows + r
    lb = np.asarray(lag_bin, np.int64)[hop.trow]
    return (B, n_bins, n_rela_rows), np.where(lb < n_bins, (b * n_bins + lb) * n_rela_rows + r, -1)


def cell_sums(shape, cell, values):
    """values summed per cell (edges with cell -1 left out), in the values' dtype."""
    values = np.asarray(values)
    out = np.zeros(int(np.prod(shape)), values.dtype)
    np.add.at(out, cell[cell >= 0], values[cell >= 0])
    return out.reshape(shape)


def expected_profile(hop, alpha_f32, B, n_rela_rows, kind="static", lag_bin=None, n_bins=None):
    """(sum int64, count int64) in profile_cells' layout from the hop's edges and their float32 alphas: sum = the integers
    rint(alpha * 2^32) added up, count = the number of edges."""
    shape, cell = profile_cells(hop, B, n_rela_rows, kind, lag_bin, n_bins)
    return cell_sums(shape, cell, fixed_point(alpha_f32)), cell_sums(shape, cell, np.ones(len(cell), np.int64))


# ---- alpha: fp64, its bound, and the one-hot readout of the forward -------------------------------------------------------------------------
def alpha_ref(case, hop, x):
    """(alpha fp64, kappa, bound) per edge of the hop for the inputs ``x`` (layer_ref.inputs)."""
    f64 = lr.forward(hop, *(x[k] for k in KEYS))
    c = lambda a: np.asarray(a, np.float64)
    kap = lr.kappa(hop, c(x["a_s"]), c(x["a_r"]), c(x["a_q"]), c(x["w_alpha"]), c(x["b_alpha"]), f64.alpha)
    return f64.alpha, kap, alpha_bound(case, kap)


def alpha_bound(case, kap):
    return lr.bound(kap, 1, lr.n0_of("agg", case.d, case.attn_dim), lr.C_BOUND)


def alpha_ratio(alpha, alpha64, kap, case):
    """The c that alpha_bound would need for these alphas (layer_ref.worst_ratio of the single-term form)."""
    return lr.worst_ratio(alpha, alpha64, kap, 1, lr.n0_of("agg", case.d, case.attn_dim))


def one_hot_tables(case, x):
    """``x`` with hidden = 0, time table = 0 and rela[row of r, r % d] = 1 in every direction's block: the forward then writes
    agg[o, r % d] = sum of the alphas of o's in-edges with that r % d."""
    y = dict(x)
    y["hidden"] = np.zeros_like(x["hidden"])
    y["time_tab"] = None if x["time_tab"] is None else np.zeros_like(x["time_tab"])
    rela = np.zeros_like(x["rela"])
    rows = np.arange(len(rela))
    rela[rows, (rows % case.n_rela_rows) % case.d] = 1.0
    y["rela"] = rela
    return y


def singleton_mask(hop, d):
    """Edges that are alone in their (new node, r % d) group."""
    key = np.asarray(hop.o, np.int64) * d + np.asarray(hop.r, np.int64) % d
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return cnt[inv] == 1
