"""explain.PathSet / RuleTable / rules_from_paths on hand-made path sets, and top_paths' argument errors (no GPU)."""
import numpy as np
import pytest
import torch

from red_gnn_amd.explain import PathSet, RDigraph, RuleTable, rules_from_paths

N_REL = 3                    # relations 0..2, inverses 3..5, identity 6


def _digraph(n_hops=2, **kw):
    # row 0: s=0 -r0-> 1 -r4-> 9, s=0 -r1-> 2 -r4-> 9, s=0 -r0-> 2;  row 1: s=5 -r6-> 5 -r2-> 7;  row 2: nothing
    edges = torch.tensor([[0, 1, 0, 0, 1], [0, 1, 0, 1, 2], [0, 1, 0, 0, 2], [0, 2, 1, 4, 9], [0, 2, 2, 4, 9],
                          [1, 1, 5, 6, 5], [1, 2, 5, 2, 7]], dtype=torch.int32)
    alpha = torch.tensor([0.5, 0.25, 0.75, 1.0, 0.5, 0.125, 0.5], dtype=torch.float32)
    args = dict(edges=edges, alpha=alpha, offsets=torch.tensor([0, 5, 7, 7]), reached=torch.tensor([True, True, False]),
                score=torch.zeros(3), n_hops=n_hops)
    args.update(kw)
    return RDigraph(**args)


def _paths(rd=None):
    rd = rd or _digraph()
    edge = torch.tensor([[[0, 3], [2, 4], [1, 4]], [[5, 6], [-1, -1], [-1, -1]], [[-1, -1]] * 3])
    product = torch.tensor([[0.5, 0.375, 0.125], [0.0625, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    return PathSet(edge=edge, product=product, count=torch.tensor([3, 1, 0], dtype=torch.int32), digraph=rd)


def _same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "support", "fixed")) and a.n_rel == b.n_rel


def test_pathset_gathers():
    ps = _paths()
    assert ps.rels().tolist() == [[[0, 4], [0, 4], [1, 4]], [[6, 2], [-1, -1], [-1, -1]], [[-1, -1]] * 3]
    assert ps.entities().tolist() == [[[0, 1, 9], [0, 2, 9], [0, 2, 9]], [[5, 5, 7], [-1] * 3, [-1] * 3], [[-1] * 3] * 3]
    assert ps.alphas().tolist() == [[[0.5, 1.0], [0.75, 0.5], [0.25, 0.5]], [[0.125, 0.5], [0.0, 0.0], [0.0, 0.0]], [[0.0, 0.0]] * 3]
    with pytest.raises(ValueError):
        ps.times()
    with pytest.raises(ValueError):
        ps.data_rows()
    t = _paths(_digraph(time=torch.arange(10, 17, dtype=torch.int32), q_time=torch.zeros(3, dtype=torch.int32),
                        data_row=torch.tensor([4, 5, 6, 7, 8, -1, 9], dtype=torch.int32)))
    assert t.times()[0].tolist() == [[10, 13], [12, 14], [11, 14]] and t.times()[1, 1].tolist() == [-1, -1]
    assert t.data_rows()[1].tolist() == [[-1, 9], [-1, -1], [-1, -1]]
    empty = PathSet(edge=torch.full((2, 1, 2), -1), product=torch.zeros((2, 1), dtype=torch.float64),
                    count=torch.zeros(2, dtype=torch.int32),
                    digraph=RDigraph(torch.zeros((0, 5), dtype=torch.int32), torch.zeros(0), torch.zeros(3, dtype=torch.int64),
                                     torch.zeros(2, dtype=torch.bool), torch.zeros(2), 2))
    assert (empty.rels() == -1).all() and (empty.entities() == -1).all() and empty.entities().shape == (2, 1, 3)


def test_rules_from_paths():
    t = rules_from_paths(_paths(), [1, 2, 0], N_REL)
    # rows 0's paths: bodies (0,4) twice and (1,4); row 1: (6,2); row 2 and the absent slots count for nothing
    assert t.head.tolist() == [1, 1, 2] and t.body.tolist() == [[0, 4], [1, 4], [6, 2]]
    assert t.support.tolist() == [2, 1, 1]
    assert t.fixed.tolist() == [int(0.875 * 2 ** 32), int(0.125 * 2 ** 32), int(0.0625 * 2 ** 32)]
    assert t.product_sum().tolist() == [0.875, 0.125, 0.0625] and t.mean().tolist() == [0.4375, 0.125, 0.0625]
    assert t.support.sum() == _paths().count.sum()
    # each path is rounded once, to the nearest unit of 2^-32 (halves up)
    ps = _paths()
    ps.product[0] = torch.tensor([1.5 * 2.0 ** -32, 2.0 ** -33, 0.49 * 2.0 ** -32], dtype=torch.float64)
    assert rules_from_paths(ps, [1, 2, 0], N_REL).fixed.tolist() == [3, 0, int(0.0625 * 2 ** 32)]
    with pytest.raises(ValueError):
        rules_from_paths(_paths(), [1, 2], N_REL)
    with pytest.raises(ValueError):
        rules_from_paths(_paths(), [1, 2, 7], N_REL)
    none = rules_from_paths(PathSet(ps.edge[2:], ps.product[2:], ps.count[2:], ps.digraph), [0], N_REL)
    assert none.head.numel() == 0 and none.body.shape == (0, 2) and none.format() == []


def test_add_is_the_table_of_the_concatenation():
    rng = np.random.default_rng(0)
    rd = _digraph()
    B, k, E = 40, 3, rd.edges.shape[0]
    edge = torch.from_numpy(rng.integers(0, E, (B, k, 2)))
    count = torch.from_numpy(rng.integers(0, k + 1, B).astype(np.int32))
    edge[torch.arange(k)[None, :] >= count[:, None]] = -1
    product = torch.from_numpy(rng.uniform(0, 1, (B, k)))
    q = rng.integers(0, 2 * N_REL, B)
    whole = rules_from_paths(PathSet(edge, product, count, rd), q, N_REL)
    parts = None
    for lo, hi in ((0, 7), (7, 8), (8, 30), (30, 40)):
        p = rules_from_paths(PathSet(edge[lo:hi], product[lo:hi], count[lo:hi], rd), q[lo:hi], N_REL)
        parts = p if parts is None else parts + p
    assert _same(whole, parts) and whole.support.sum() == count.sum()
    key = torch.cat([whole.head[:, None], whole.body], 1).tolist()
    assert key == sorted(key) and len({tuple(x) for x in key}) == len(key)
    empty = rules_from_paths(PathSet(edge[:0], product[:0], count[:0], rd), q[:0], N_REL)
    assert _same(whole + empty, whole) and _same(empty + whole, whole) and _same(whole.cpu(), whole)
    with pytest.raises(ValueError):
        whole + RuleTable(whole.head, whole.body, whole.support, whole.fixed, N_REL + 1)
    with pytest.raises(ValueError):
        whole + RuleTable(whole.head, whole.body[:, :1], whole.support, whole.fixed, N_REL)


def test_top_and_format():
    head = torch.tensor([0, 0, 0, 0, 4])
    body = torch.tensor([[0, 1], [1, 6], [2, 5], [6, 6], [3, 0]])
    t = RuleTable(head, body, torch.tensor([2, 5, 5, 1, 9]), torch.tensor([2, 5, 5, 1, 9]) << 30, N_REL)
    top = t.top(0, 3)
    assert top.body.tolist() == [[1, 6], [2, 5], [0, 1]] and top.support.tolist() == [5, 5, 2] and top.head.tolist() == [0, 0, 0]
    assert t.top(0, 10).support.tolist() == [5, 5, 2, 1] and t.top(2, 3).head.numel() == 0
    with pytest.raises(ValueError):
        t.top(0, 0)
    assert t.format() == ["r0(x,z1) ^ r1(z1,y) -> r0(x,y)", "r1(x,y) -> r0(x,y)", "r2(x,z1) ^ r2^-1(z1,y) -> r0(x,y)",
                          "x=y -> r0(x,y)", "r0^-1(x,z1) ^ r0(z1,y) -> r1^-1(x,y)"]
    assert t.format(id2rel=["father", "mother", "wife"])[2] == "wife(x,z1) ^ wife^-1(z1,y) -> father(x,y)"
    assert t.format(id2rel={0: "father", 1: "mother", 2: "wife"})[4] == "father^-1(x,z1) ^ father(z1,y) -> mother^-1(x,y)"


def test_top_paths_argument_errors_before_the_device():
    rd = _digraph()
    for k in (0, 9, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            rd.top_paths(k)
    with pytest.raises(ValueError, match="scratch_bytes"):
        rd.top_paths(1, scratch_bytes=-1)
    for bad in (dict(edges=rd.edges.long()), dict(edges=rd.edges[:, :4]), dict(alpha=rd.alpha.double()), dict(alpha=rd.alpha[:-1]),
                dict(offsets=rd.offsets.int()), dict(offsets=rd.offsets.reshape(2, 2)), dict(n_hops=0), dict(n_hops=33)):
        with pytest.raises(ValueError, match="top_paths: (edges|alpha|offsets|n_hops) must be"):
            _digraph(**bad).top_paths(2)
    for off in ([0, 5, 4, 7], [0, 5, 7, 6], [0, 5, 7, 8], [1, 5, 7, 7], [-1, 5, 7, 7]):
        with pytest.raises(ValueError, match="offsets must start at 0"):
            _digraph(offsets=torch.tensor(off)).top_paths(2)
    with pytest.raises(ValueError, match="needs the digraph on the device"):
        rd.top_paths(2)
