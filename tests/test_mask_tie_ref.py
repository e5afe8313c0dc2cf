"""Tied edge masks without a GPU: explain.mask_groups against the plain-Python grouping of tests/mask_tie_ref.py on the four cases of
tests/rescore_ref.py and on a hand-built digraph (every array, both named ties and a label tie); the conditions the fixtures are
chosen for, asserted; tie="fact" against _FactSums._fact_sums, whose grouping is fact_mask's rule; the ValueErrors of ``tie`` and
where they fall in learn_mask's order of checks; the new symbols in the header and in the binding; a tied EdgeMask built by hand."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

from tests import mask_tie_ref as TR
from tests import rescore_ref as R
from tests.test_fidelity_host import EDGES, N_REL, _cpu_model, _digraph
from tests.test_tfidelity_host import _tdigraph

_CASES = {}


def _case(name):
    """The case and its digraph as a CPU RDigraph: computed once, shared, left as it is."""
    if name not in _CASES:
        from red_gnn_amd.explain import RDigraph
        c = R.make_case(name, **R.CASES[name])
        E = len(c.edges)
        rd = RDigraph(edges=torch.as_tensor(c.edges).to(torch.int32), alpha=torch.zeros(E), offsets=torch.as_tensor(c.offsets),
                      reached=torch.ones(c.B, dtype=torch.bool), score=torch.zeros(c.B), n_hops=c.L, q_sub=torch.as_tensor(c.subs),
                      q_rel=torch.as_tensor(c.rels), n_rel=c.n_rel)
        _CASES[name] = (c, rd)
    return _CASES[name]


def _same(tag, got, want, B):
    assert got.group_of.dtype == torch.int32 and got.grp_ptr.dtype == torch.int32 and got.member.dtype == torch.int32, tag
    assert got.row_ptr.dtype == got.group_row.dtype == got.group_key.dtype == torch.int64, tag
    assert got.group_of.tolist() == want.group_of.tolist(), tag + ": group_of"
    assert got.grp_ptr.tolist() == want.grp_ptr.tolist() and got.grp_ptr_host.tolist() == want.grp_ptr.tolist(), tag + ": grp_ptr"
    assert got.grp_ptr_host.dtype == np.int32 and got.member.tolist() == want.member.tolist(), tag + ": member"
    assert got.row_ptr.tolist() == TR.row_ptr(want.group_row, B).tolist(), tag + ": row_ptr"
    assert got.group_row.tolist() == want.group_row.tolist() and got.group_key.tolist() == want.group_key.tolist(), tag + ": keys"
    assert tuple(got.group_key.shape) == tuple(want.group_key.shape) and got.n_groups == want.n_groups, tag


def _label_tie(c, rng):
    """A label per edge (hop * (2 n_rel + 1) + rel is "relation" again; the tail entity is another question), a free set of about
    four fifths of the facts' edges, and -1 wherever the edge is not free: labels there are not read."""
    e = c.edges
    free = (e[:, 3] != 2 * c.n_rel) & (rng.random(len(e)) < 0.8)
    return np.where(free, e[:, 4], -1).astype(np.int64), free


@pytest.mark.parametrize("name", list(R.CASES))
def test_mask_groups_is_the_reference_grouping(name):
    from red_gnn_amd.explain import mask_groups
    c, rd = _case(name)
    facts = c.edges[:, 3] != 2 * c.n_rel
    for tie in ("fact", "relation"):
        _same("%s %s" % (name, tie), mask_groups(rd, tie, torch.as_tensor(facts)), TR.groups(c.edges, c.n_rel, tie, facts), c.B)
    label, free = _label_tie(c, np.random.default_rng(5))
    want = TR.groups(c.edges, c.n_rel, label, free)
    assert 0 < want.n_groups < free.sum() and not free.all()
    _same(name + " labels (numpy)", mask_groups(rd, label, free), want, c.B)
    _same(name + " labels (tensor)", mask_groups(rd, torch.as_tensor(label), torch.as_tensor(free)), want, c.B)
    # a label tie carrying (hop, rel) in one number is "relation"
    both = c.edges[:, 1] * (2 * c.n_rel + 1) + c.edges[:, 3]
    a, b = mask_groups(rd, torch.as_tensor(both), torch.as_tensor(facts)), mask_groups(rd, "relation", torch.as_tensor(facts))
    assert torch.equal(a.group_of, b.group_of) and torch.equal(a.member, b.member) and torch.equal(a.grp_ptr, b.grp_ptr)
    # a self-loop is no fact: never tied under "fact", a group like any other under the other ties
    every = np.ones(len(c.edges), bool)
    assert mask_groups(rd, "fact", every).group_of.tolist() == TR.groups(c.edges, c.n_rel, "fact", facts).group_of.tolist()
    _same(name + " relation, all edges", mask_groups(rd, "relation", every), TR.groups(c.edges, c.n_rel, "relation", every), c.B)
    # nothing free: no groups
    none = mask_groups(rd, "fact", ~every)
    assert none.n_groups == 0 and none.grp_ptr.tolist() == [0] and not (none.group_of >= 0).any() and none.row_ptr.tolist() == [0] * (c.B + 1)
    assert tuple(none.group_key.shape) == (0, 3) and none.member.numel() == 0


def test_the_fixtures_hold_what_they_are_chosen_for():
    """e300_L3 and e60_L3 hold facts of 2-4 edges (the same fact at several hops, and its inverse); e300_L2's facts are one edge each,
    so there a tied mask has to be the untied one."""
    sizes = {}
    for name in R.CASES:
        c, _ = _case(name)
        T = TR.groups(c.edges, c.n_rel, "fact", c.edges[:, 3] != 2 * c.n_rel)
        sizes[name] = np.diff(T.grp_ptr)
        assert sizes[name].min() >= 1
    for name in ("e300_L3", "e60_L3"):
        assert (sizes[name] >= 2).sum() >= 30 and sizes[name].max() in (3, 4), (name, np.bincount(sizes[name]))
    assert (sizes["e60_L2"] >= 2).any()
    assert (sizes["e300_L2"] == 1).all()
    c, _ = _case("e300_L2")
    assert not (c.edges[:, 3] == 2 * c.n_rel).any()                           # ... and it has no self-loop
    # "relation" cuts coarser: groups of many edges
    c, _ = _case("e300_L3")
    assert np.diff(TR.groups(c.edges, c.n_rel, "relation", c.edges[:, 3] != 2 * c.n_rel).grp_ptr).max() > 4


# one row (s = 5, o = 5): the fact 5 -r0-> 6 at hops 1 and 2, its inverse at hop 3, another fact 5 -r1-> 6 at hop 2, and self-loops
HAND = [[0, 1, 5, 6, 5], [0, 1, 5, 0, 6], [0, 2, 5, 0, 6], [0, 2, 5, 1, 6], [0, 2, 6, 6, 6], [0, 3, 6, 3, 5], [0, 3, 5, 6, 5],
        [1, 1, 5, 0, 6]]


def test_mask_groups_on_a_hand_built_digraph():
    from red_gnn_amd.explain import mask_groups
    rd = _digraph(HAND, 2, n_hops=3)
    loops = torch.tensor(HAND)[:, 3] == 2 * N_REL
    T = mask_groups(rd, "fact", ~loops)
    assert T.group_of.tolist() == [-1, 0, 0, 1, -1, 0, -1, 2]
    assert T.grp_ptr.tolist() == [0, 3, 4, 5] and T.member.tolist() == [1, 2, 5, 3, 7]
    assert T.group_row.tolist() == [0, 0, 1] and T.group_key.tolist() == [[5, 0, 6], [5, 1, 6], [5, 0, 6]]
    assert T.row_ptr.tolist() == [0, 2, 3] and T.n_groups == 3
    _same("hand fact", T, TR.groups(HAND, N_REL, "fact", (~loops).numpy()), 2)
    T = mask_groups(rd, "relation", ~loops)                                   # (hop, rel): (1, 0), (2, 0), (2, 1), (3, 3) | (1, 0)
    assert T.group_of.tolist() == [-1, 0, 1, 2, -1, 3, -1, 4] and T.group_key.tolist() == [[1, 0], [2, 0], [2, 1], [3, 3], [1, 0]]
    assert T.row_ptr.tolist() == [0, 4, 5]
    _same("hand relation", T, TR.groups(HAND, N_REL, "relation", (~loops).numpy()), 2)
    label = torch.tensor([-1, 7, 3, 7, -5, 3, -1, 7])                         # negative labels where the edge is not free
    T = mask_groups(rd, label, ~loops)
    assert T.group_of.tolist() == [-1, 1, 0, 1, -1, 0, -1, 2] and T.member.tolist() == [2, 5, 1, 3, 7] and T.group_key.tolist() == [[3], [7], [7]]
    _same("hand labels", T, TR.groups(HAND, N_REL, label.numpy(), (~loops).numpy()), 2)


@pytest.mark.parametrize("name", ["e60_L3", "e300_L2"])
def test_fact_groups_are_the_fact_sums_grouping(name):
    from red_gnn_amd.explain import Saliency, mask_groups
    c, rd = _case(name)
    E = len(c.edges)
    facts = torch.as_tensor(c.edges[:, 3] != 2 * c.n_rel)
    T = mask_groups(rd, "fact", facts)
    value = torch.arange(1, E + 1, dtype=torch.float32)                       # small integers: exact in any order
    sal = Saliency(score=rd.score, reached=rd.reached, live=torch.ones(E, dtype=torch.bool), alpha=rd.alpha, edge_grad=value, digraph=rd)
    row, fact, total = sal.fact_grad()
    assert torch.equal(row, T.group_row) and torch.equal(fact, T.group_key)
    want = TR.group_sums32(T.grp_ptr.numpy(), T.member.numpy(), value.numpy()[None, :])[0]
    assert np.array_equal(total.numpy(), want)
    assert np.array_equal(want, TR.group_sums64(T.grp_ptr.numpy(), T.member.numpy(), value.numpy()[None, :])[0])
    # ... which is fact_mask's rule: a group's members are the edges fact_mask marks for its fact in its row
    for g in range(0, T.n_groups, max(1, T.n_groups // 7)):
        mask = rd.fact_mask(T.group_key[g][None, :], rows=T.group_row[g][None])
        assert torch.nonzero(mask).reshape(-1).tolist() == T.member[T.grp_ptr[g]:T.grp_ptr[g + 1]].tolist()


def test_group_sums_reference_follows_the_definition():
    x = np.array([[1.0, 2.0 ** -24, 2.0 ** -24, -0.0]], np.float32)
    ptr, member = np.array([0, 3, 3, 4], np.int32), np.array([0, 1, 2, 3], np.int32)
    got = TR.group_sums32(ptr, member, x, chunk=32)
    assert got.tolist() == [[1.0, 0.0, -0.0]] and np.signbit(got[0, 2]) and not np.signbit(got[0, 1])     # one member: its own bits
    # member by member both halves of an ulp are lost; in chunks of two, (2^-24 + 2^-24) + (1) keeps them: the cut is part of the bits
    one = np.array([0, 3], np.int32)
    assert TR.group_sums32(one, member, x, chunk=1)[0, 0] == 1.0 and TR.group_sums32(one, member[[1, 2, 0]], x, chunk=2)[0, 0] > 1.0
    assert TR.group_sums32(one, member[[1, 2, 0]], x, chunk=32)[0, 0] > 1.0 and TR.group_sums32(one, member[[1, 0, 2]], x, chunk=32)[0, 0] == 1.0


def test_tie_is_checked_with_the_other_arguments_in_order():
    from red_gnn_amd import explain
    model, rd = _cpu_model(), _digraph(EDGES, 2)
    for tie in ("facts", "", 3, 1.5, True, [0] * 9, ("fact",), object()):
        with pytest.raises(ValueError, match="learn_mask: tie"):
            rd.learn_tied_mask(model, tie=tie)
        with pytest.raises(ValueError, match="learn_mask: tie"):
            explain.learn_mask(rd, model, tie=tie)
    # the other arguments of learn_mask come first, the timed refusal and the digraph's tensors after
    with pytest.raises(ValueError, match="learn_mask: theta0"):
        rd.learn_tied_mask(model, tie="facts", theta0=float("nan"))
    with pytest.raises(ValueError, match="learn_mask: tie"):
        _tdigraph().learn_tied_mask(model, tie="facts")
    with pytest.raises(ValueError, match="learn_mask: .*timed forms are not built"):
        _tdigraph().learn_tied_mask(model, tie="fact")
    with pytest.raises(ValueError, match="learn_mask: .*timed forms are not built"):
        _tdigraph().learn_tied_mask(model, tie=torch.zeros(3))                # a tensor tie needs E: checked after the digraph
    with pytest.raises(ValueError, match="learn_mask: alpha must be float32"):
        _digraph(EDGES, 2, alpha=torch.zeros(8)).learn_tied_mask(model, tie=torch.zeros(3))
    for tie in (torch.zeros(9), torch.zeros(9, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), torch.zeros((9, 1), dtype=torch.int64),
                np.zeros(9, np.int32), np.zeros(10, np.int64)):
        with pytest.raises(ValueError, match="learn_mask: tie must be int64 \\[9\\]"):
            rd.learn_tied_mask(model, tie=tie)
    with pytest.raises(ValueError, match="learn_mask: tie must be int64"):    # ... and before keep's and the model's
        rd.learn_tied_mask(model, tie=torch.zeros(9), keep=torch.ones(9))
    with pytest.raises(ValueError, match="learn_mask: keep must be bool"):
        rd.learn_tied_mask(model, tie="fact", keep=torch.ones(9))
    for tie in ("fact", "relation", torch.zeros(9, dtype=torch.int64), np.arange(9)):
        with pytest.raises(ValueError, match="learn_mask: .*on one device"):  # all in order: then the device is asked for
            rd.learn_tied_mask(model, tie=tie, iterations=0)
    # mask_groups' own: the labels of the free edges, the shape of free
    loops = torch.tensor(EDGES)[:, 3] == 2 * N_REL
    with pytest.raises(ValueError, match="learn_mask: tie holds a negative label"):
        explain.mask_groups(rd, torch.where(loops, 0, -1), ~loops)
    with pytest.raises(ValueError, match="learn_mask: tie None"):
        explain.mask_groups(rd, None, ~loops)
    with pytest.raises(ValueError, match="learn_mask: free"):
        explain.mask_groups(rd, "fact", torch.ones(8, dtype=torch.bool))
    with pytest.raises(ValueError, match="learn_mask: tie"):
        explain.mask_groups(rd, "hop", ~loops)


def test_signatures_and_bindings():
    from red_gnn_amd import _lib, engine, explain
    from red_gnn_amd.models import RED_GNN_induc, RED_GNN_trans
    assert inspect.signature(explain.learn_mask).parameters["tie"].default is None
    assert inspect.signature(RED_GNN_trans.learn_mask).parameters["tie"].default is None
    assert list(inspect.signature(explain.RDigraph.learn_tied_mask).parameters)[1:3] == ["model", "tie"]
    assert "kw" in inspect.signature(RED_GNN_induc.learn_mask).parameters
    names = ("rg_mask_tie_grad_scratch_bytes", "rg_mask_tie_grad", "rg_mask_tie_gates")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "redgnn.h")).read()
    for name in names:
        assert name in _lib.SYMBOLS and ("%s(" % name) in header, name
    assert "#define RG_MASK_TIE_CHUNK %d" % engine.MASK_TIE_CHUNK in header and engine.MASK_TIE_CHUNK == 32
    L = _lib.lib()
    assert L.rg_version() == 12
    assert len(L.rg_mask_tie_grad.argtypes) == 12 and len(L.rg_mask_tie_gates.argtypes) == 7
    assert len(L.rg_mask_tie_grad_scratch_bytes.argtypes) == 3 and len(L.rg_mask_step.argtypes) == 24
    for name in names:
        assert hasattr(L, name)
    # the scratch rule needs no device: nothing while no group is cut, then the chunk list and a partial sum per (replica, chunk)
    ptr = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert L.rg_mask_tie_grad_scratch_bytes(_lib.ptr(ptr([0, 1, 32, 32])), 4, 3) == 0
    one, two = (int(L.rg_mask_tie_grad_scratch_bytes(_lib.ptr(ptr([33, 1, 1025])), 3, r)) for r in (1, 64))
    assert one > 0 and two - one == 256 * ((64 * 35 * 4 + 255) // 256) - 256
    for f in (engine.mask_tie_grad, engine.mask_tie_gates, explain.mask_groups):
        assert callable(f)


def _tied_mask(tie, key, gate, row):
    from red_gnn_amd.explain import EdgeMask
    z = torch.zeros(2)
    e = torch.zeros(9)
    return EdgeMask(gate=e, keep=e.bool(), score=torch.tensor([1.0, 2.0]), hard_score=z, kept_score=z, target=z, baseline_score=z,
                    size=torch.tensor([1, 1]), n_free=torch.tensor([2, 3]), replica=torch.tensor([0, 1]), lambdas=torch.tensor([0.1, 0.3]),
                    history=types.SimpleNamespace(), reached=torch.tensor([True, True]), live=e.bool(), digraph=_digraph(EDGES, 2),
                    tie=tie, group=torch.zeros(9, dtype=torch.int64), group_row=torch.tensor(row), group_key=torch.tensor(key),
                    group_gate=torch.tensor(gate), n_groups=torch.bincount(torch.tensor(row), minlength=2))


def test_edge_mask_groups_and_format_groups():
    mk = _tied_mask("relation", [[1, 3], [2, 0], [2, 7], [1, 3]], [0.984, 0.25, 0.906, 0.5], [0, 0, 0, 1])
    row, key, gate = mk.groups()
    assert row.tolist() == [0, 0, 0, 1] and key.tolist() == [[1, 3], [2, 0], [2, 7], [1, 3]] and gate.dtype == torch.float32
    assert mk.format_groups() == ["row 0: hop1 r3 0.98  hop2 r7 0.91  hop2 r0 0.25", "row 1: hop1 r3 0.50"]
    assert mk.format_groups(k=2)[0] == "row 0: hop1 r3 0.98  hop2 r7 0.91"
    names = ["r%s" % c for c in "abcdefgh"]
    assert mk.format_groups(id2rel=names, k=1) == ["row 0: hop1 rd 0.98", "row 1: hop1 rd 0.50"]
    mk = _tied_mask("fact", [[5, 0, 6], [5, 1, 6]], [0.75, 0.75], [1, 1])       # a tie in the gate: key order; a row without groups
    assert mk.format_groups() == ["row 0: ", "row 1: (5, r0, 6) 0.75  (5, r1, 6) 0.75"]
    mk = _tied_mask(torch.zeros(9, dtype=torch.int64), [[4], [9]], [0.125, 1.0], [0, 1])
    assert mk.format_groups() == ["row 0: 4 0.12", "row 1: 9 1.00"]
    with pytest.raises(ValueError, match="format_groups: k"):
        mk.format_groups(k=0)
    from tests.test_learn_mask_host import _mask
    with pytest.raises(ValueError, match="groups: the mask is not tied"):
        _mask().groups()
    assert _mask().tie is None and _mask().group_gate is None                 # today's constructors keep working
