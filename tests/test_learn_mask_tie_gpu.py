"""Tied edge masks on the MI355X (-m gpu), end to end: RDigraph.learn_tied_mask / explain.learn_mask(tie=) / model.learn_mask(tie=) on
the four cases of tests/rescore_ref.py and once on the inductive fixture.  Mostly conditions on bits, as tests/test_learn_mask_gpu.py
states them for the untied driver: the tied driver is rescore(gate=), saliency(gate=), engine.mask_tie_grad, engine.mask_step and
engine.mask_tie_gates put together with the replicas walked in one launch per hop, so a loop the test writes from those public pieces,
one replica at a time, has to give the same gates, iteration by iteration.  What the tie is for: under tie="fact" every copy of a
fact holds one gate, ``keep`` is a fact_mask and ``size`` counts facts; where every fact is one edge (e300_L2) the gates are the
untied driver's, bit for bit.  Against tests/mask_tie_ref.learn_tied (fp64, on ig_ref.gradient_at) under the project's stated
tolerance - rtol 1e-4 / atol 2e-5, or 4 x the fp32 restatement's own error, through tests/_util.assert_close_fp32 - the constants,
the first deviation and the group gradient at the initial gates; no gates after Adam's first step (tests/mask_ref.py says why).
As measured on an MI355X, the worst |got - ref64| over the four cases: 1.8e-7 for target, 8.8e-8 for baseline_score, 1.9e-5 for the
first deviation (e60_L2, values up to 2.5; 2.1e-6 elsewhere) and 1.8e-7 for the group gradient, next to 9.5e-8, 8.5e-8, 6.1e-6 and
6.2e-8 for the fp32 reference (information only).  Wall time of this file there: 7.4 s (26 tests)."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import mask_tie_ref as TR
from tests import rescore_ref as R
from tests.test_explain_gpu import P
from tests.test_saliency_gpu import _setup

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
LAMBDAS = (0.02, 0.2, 1.0)
KW = dict(lambdas=LAMBDAS, entropy=0.05, iterations=3, lr=0.3, theta0=1.0)
KW5 = dict(lambdas=(0.02, 5.0), entropy=0.05, iterations=5, lr=0.3, theta0=1.0)      # five steps of 0.3 carry a logit from 1 to below 0
_MASKS = {}


def _mask(name, tie, kw=KW):
    """A tied mask of a case: computed once, shared by the tests, left as it is."""
    key = (name, tie, id(kw))
    if key not in _MASKS:
        c, model, rd, e = _setup(name)
        _MASKS[key] = rd.learn_tied_mask(model, tie=tie, **kw)
    return _MASKS[key]


def _parts(rd, n_rel, keep=None):
    E = rd.edges.shape[0]
    kept = torch.ones(E, dtype=torch.bool, device="cuda") if keep is None else keep.bool()
    fixed = kept & (rd.edges[:, 3] == 2 * n_rel)
    return kept & ~fixed, fixed


def _first_member(T):
    """The first member edge of every (non-empty) group: where to read a group's gate from an edge array."""
    return T.member[T.grp_ptr[:-1].long()].long()


@pytest.mark.parametrize("name", list(R.CASES))
def test_fact_tie_makes_the_mask_a_set_of_facts(name):
    from red_gnn_amd import explain
    c, model, rd, e = _setup(name)
    mk = _mask(name, "fact", KW5)
    free, fixed = _parts(rd, c.n_rel)
    T = explain.mask_groups(rd, "fact", free)
    ref = TR.groups(e, c.n_rel, "fact", free.cpu().numpy())
    assert torch.equal(mk.group, T.group_of.long()) and np.array_equal(T.group_of.cpu().numpy(), ref.group_of)
    assert torch.equal(mk.group_row, T.group_row) and torch.equal(mk.group_key, T.group_key) and mk.tie == "fact"
    assert torch.equal(mk.n_groups, T.row_ptr[1:] - T.row_ptr[:-1]) and torch.equal(mk.n_free, torch.bincount(rd.edges[:, 0].long()[free], minlength=c.B))
    assert int(mk.n_groups.sum()) == ref.n_groups and (name == "e300_L2") == bool(torch.equal(mk.n_groups, mk.n_free))
    group = mk.group[free]
    first = _first_member(T)
    # ---- every copy of a fact holds one gate: in every replica and in the rows' selection
    for k in range(len(KW5["lambdas"])):
        g = mk.replica_gate[k]
        assert torch.equal(g[free], g[first][group]), "%s: replica %d holds a fact with two gates" % (name, k)
        assert bool((g[fixed] == 1).all())
        # the replica's hard mask is a fact_mask: the facts above 0.5 with all their copies, and the self-loops
        sel = g[first] > 0.5
        hard_keep = torch.where(free, g > 0.5, fixed)
        assert torch.equal(hard_keep, rd.fact_mask(T.group_key[sel], rows=T.group_row[sel]) | fixed), "%s: replica %d" % (name, k)
        assert torch.equal(mk.replica_size[k], torch.bincount(T.group_row[sel], minlength=c.B)), "%s: size counts facts" % name
    assert bool((mk.replica_gate[:, free] <= 0.5).any()) and bool((mk.replica_gate[:, free] > 0.5).any())      # some facts go, some stay
    assert torch.equal(mk.gate[free], mk.group_gate[group]) and torch.equal(mk.group_gate, mk.gate[first])
    sel = mk.group_gate > 0.5
    assert torch.equal(mk.keep, rd.fact_mask(T.group_key[sel], rows=T.group_row[sel]) | fixed), name + ": keep is not a fact_mask"
    assert torch.equal(mk.size, torch.bincount(T.group_row[sel], minlength=c.B)) and bool((mk.size <= mk.n_groups).all())
    assert torch.equal(mk.kept_score, rd.rescore(model, keep=mk.keep).score)
    # ---- fact_gate has no maximum left to take
    row, fact, gate = mk.fact_gate()
    assert torch.equal(row, mk.group_row) and torch.equal(fact, mk.group_key) and torch.equal(gate, mk.group_gate)
    row, key, gate = mk.groups()
    assert torch.equal(gate, mk.group_gate) and len(mk.format_groups(k=2)) == c.B and mk.format_groups(k=1)[0].startswith("row 0: (")
    # ---- the untied mask of the same settings does what the tie is there to prevent (where there is a fact with copies to split)
    if name in ("e300_L3", "e60_L3"):
        un = rd.learn_mask(model, **KW5)
        g = un.replica_gate
        assert not torch.equal(g[:, free], g[:, first][:, group]), name + ": the untied copies of a fact agree"


def _singleton_pair():
    c, model, rd, e = _setup("e300_L2")
    if "untied e300_L2" not in _MASKS:
        _MASKS["untied e300_L2"] = rd.learn_mask(model, **KW)
    return _mask("e300_L2", "fact"), _MASKS["untied e300_L2"]


def test_singleton_groups_give_the_untied_gates():
    """e300_L2: every fact is one edge and there is no self-loop, so the tied driver is the untied one, bit for bit, after three
    iterations: the sum of one member is that member's bits (tests/test_mask_tie_gpu.py) and the group arrays hold the same cells as
    the edge arrays, in (h, r, t) order instead of edge order.  Both drivers walk through explain._gated_group, which chooses the GEMM
    library of its dense adjoint itself (engine.prefer_blas): the condition does not depend on what the process ran before.  It is a
    condition on THIS case: rg_mask_step rounds a row's last n mod 4 cells differently from the cells it takes four at a time
    (DESIGN.md 4), 4 of these 44 cells change sides under the reordering, and here none of them lands on a rounding boundary."""
    tied, un = _singleton_pair()
    a, b = tied.replica_gate.cpu().numpy(), un.replica_gate.cpu().numpy()
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    print("e300_L2 tied against untied replica_gate: %d of %d cells differ, max |diff| %.3g, max %d ulp (bits: tied %s, untied %s)"
          % (int((a != b).sum()), a.size, float(np.abs(a - b).max()), int(ulp.max()), U.sha(a)[:12], U.sha(b)[:12]))
    assert torch.equal(tied.replica_gate, un.replica_gate) and torch.equal(tied.gate, un.gate) and torch.equal(tied.keep, un.keep)
    for field in ("score", "hard_score", "kept_score", "target", "baseline_score", "size", "replica", "replica_size", "n_free", "reached"):
        assert torch.equal(getattr(tied, field), getattr(un, field)), field
    assert torch.equal(tied.n_groups, un.n_free)
    assert torch.equal(tied.history.deviation, un.history.deviation) and torch.equal(tied.history.count, un.history.count)
    assert float((tied.replica_gate[0] - tied.replica_gate[2]).abs().max()) > 1e-3


def test_the_walks_gemm_library_is_chosen_per_replica(monkeypatch):
    """explain._gated_group chooses the GEMM library of its dense adjoint from a row count (engine.prefer_blas, which switches at 2^17
    rows).  The count has to be one replica's - the hop's destination nodes - and never the stacked rows: a replica of a stacked call
    is promised the bits of its own one-replica call, so both must get the same library at every size, also where n_dst < 2^17 <=
    R * n_dst, which no test case reaches.  The arguments are recorded: those of a three-replica call are those of a one-replica call."""
    from red_gnn_amd import engine
    c, model, rd, e = _setup("e60_L3")
    seen = []
    monkeypatch.setattr(engine, "prefer_blas", lambda n, _f=engine.prefer_blas: (seen.append(int(n)), _f(n))[1])
    calls = {}
    for lambdas in ((0.2,), LAMBDAS):
        for tie in (None, "fact"):
            del seen[:]
            (rd.learn_mask(model, **dict(KW, lambdas=lambdas, iterations=1)) if tie is None else
             rd.learn_tied_mask(model, tie=tie, **dict(KW, lambdas=lambdas, iterations=1)))
            calls[len(lambdas), tie] = list(seen)
    assert calls[1, None] and calls[3, None] == calls[1, None] == calls[3, "fact"] == calls[1, "fact"]
    del seen[:]
    rd.saliency(model, gate=torch.ones(len(e), device="cuda"))                # one walk, forward and adjoint: every hop twice
    nodes = [int(torch.unique(rd.edges[rd.edges[:, 1] == l][:, [0, 4]].long(), dim=0).shape[0]) for l in range(1, c.L + 1)]
    assert seen == nodes + nodes[::-1], (seen, nodes)
    del seen[:]
    rd.integrated_gradients(model, steps=4)                                   # replicas on stacked rows: still the hop's own count
    assert set(seen) <= set(nodes) and seen


@pytest.mark.parametrize("tie", ["fact", "relation"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_three_iterations_are_the_loop_of_the_public_pieces(name, tie):
    from red_gnn_amd import engine, explain
    c, model, rd, e = _setup(name)
    mk = _mask(name, tie)
    free, fixed = _parts(rd, c.n_rel)
    E, B = len(e), c.B
    T = explain.mask_groups(rd, tie, free)
    G = T.n_groups
    scale = (mk.target - mk.baseline_score).abs()
    inv_scale = torch.where((scale > 0) & mk.reached, 1.0 / scale, torch.zeros_like(scale))
    inv_n = torch.where(mk.n_groups > 0, 1.0 / mk.n_groups.to(torch.float32), torch.zeros(B, device="cuda"))
    assert torch.equal(mk.target, rd.rescore(model, gate=torch.ones(E, device="cuda")).score)
    assert torch.equal(mk.baseline_score, rd.rescore(model, gate=fixed.float()).score)
    g0 = float(np.float32(1.0 / (1.0 + np.exp(-KW["theta0"]))))
    every = torch.ones(G, dtype=torch.bool, device="cuda")
    for k, lam in enumerate(LAMBDAS):
        theta = torch.full((1, G), KW["theta0"], device="cuda")
        m, v = torch.zeros((1, G), device="cuda"), torch.zeros((1, G), device="cuda")
        grp_gate = torch.full((1, G), g0, device="cuda")
        gate = torch.where(free, torch.full((E,), g0, device="cuda"), fixed.float())[None, :].contiguous()
        lam_s, lam_e = torch.tensor([lam], device="cuda"), torch.tensor([KW["entropy"]], device="cuda")
        for it in range(KW["iterations"]):
            sal = rd.saliency(model, gate=gate[0].contiguous())
            tag = "%s %s lambda %g iteration %d" % (name, tie, lam, it)
            assert torch.equal(mk.history.deviation[it, k], (sal.score - mk.target) * inv_scale), tag + ": deviation"
            grp_grad = engine.mask_tie_grad(T.grp_ptr, T.member, sal.edge_grad[None, :].contiguous(), G, grp_ptr_host=T.grp_ptr_host)
            grp_gate, size, count = engine.mask_step(T.row_ptr, every, sal.score[None, :].contiguous(), mk.target, inv_scale, inv_n, lam_s,
                                                     lam_e, grp_grad, theta, m, v, it + 1, lr=KW["lr"], gate_out=grp_gate)
            engine.mask_tie_gates(T.group_of, grp_gate, gate)
            assert torch.equal(mk.history.size[it, k], size[0]) and torch.equal(mk.history.count[it, k], count[0]), tag + ": size / count"
        assert torch.equal(mk.replica_gate[k], gate[0]), "%s %s lambda %g: the final gates" % (name, tie, lam)
        assert torch.equal(mk.replica_score[k], rd.rescore(model, gate=gate[0].contiguous()).score)
        hard = torch.where(free, (gate[0] > 0.5).float(), gate[0])
        assert torch.equal(mk.replica_hard_score[k], rd.rescore(model, gate=hard).score)
        assert torch.equal(mk.replica_size[k], torch.bincount(T.group_row[grp_gate[0] > 0.5], minlength=B))
    assert float((mk.replica_gate[0] - mk.replica_gate[2]).abs().max()) > 1e-3                  # the lambdas matter
    # ---- a replica of the stacked call is its own call, and two calls give the same bits
    one = rd.learn_tied_mask(model, tie=tie, **dict(KW, lambdas=(LAMBDAS[1],)))
    assert torch.equal(one.gate, mk.replica_gate[1]) and torch.equal(one.group_gate, mk.replica_gate[1][_first_member(T)])
    for field in ("deviation", "size", "count"):
        assert torch.equal(getattr(one.history, field)[:, 0], getattr(mk.history, field)[:, 1]), field
    again = rd.learn_tied_mask(model, tie=tie, **KW)
    for field in ("gate", "keep", "score", "hard_score", "kept_score", "size", "replica", "group_gate"):
        assert torch.equal(getattr(again, field), getattr(mk, field)), field
    assert torch.equal(mk.gate, mk.replica_gate[mk.replica[rd.edges[:, 0].long()], torch.arange(E, device="cuda")])
    assert torch.equal(mk.keep, torch.where(free, mk.gate > 0.5, fixed)) and torch.equal(mk.kept_score, rd.rescore(model, keep=mk.keep).score)


@pytest.mark.parametrize("name", list(R.CASES))
def test_constants_first_deviation_and_group_gradient_against_the_reference(name):
    from red_gnn_amd import engine, explain
    c, model, rd, e = _setup(name)
    mk = _mask(name, "fact")
    ref = {dt: TR.learn_tied(c.params, e, c.subs, c.rels, c.n_ent, c.n_rel, c.L, c.act, LAMBDAS[0], KW["entropy"], 1, KW["lr"], KW["theta0"],
                             "fact", dtype=dt) for dt in (np.float64, np.float32)}
    r64, r32 = ref[np.float64], ref[np.float32]
    # the group gradient at the initial gates: the chain rule through the tie, from the public pieces
    free, fixed = _parts(rd, c.n_rel)
    T = explain.mask_groups(rd, "fact", free)
    g0 = float(np.float32(1.0 / (1.0 + np.exp(-KW["theta0"]))))
    gate0 = torch.where(free, torch.full((len(e),), g0, device="cuda"), fixed.float())
    sal = rd.saliency(model, gate=gate0)
    grp_grad = engine.mask_tie_grad(T.grp_ptr, T.member, sal.edge_grad[None, :].contiguous(), T.n_groups, grp_ptr_host=T.grp_ptr_host)[0]
    assert np.array_equal(T.group_of.cpu().numpy(), r64["groups"].group_of)
    for field, got, want32, want64 in (("target", mk.target, r32["target"], r64["target"]),
                                       ("baseline_score", mk.baseline_score, r32["baseline_score"], r64["baseline_score"]),
                                       ("deviation", mk.history.deviation[:1, 0], r32["deviation"], r64["deviation"]),
                                       ("group_grad", grp_grad, r32["group_grad"][0], r64["group_grad"][0])):
        got = got.cpu().numpy()
        print("%s %s: max |got - ref64| %.3g (ref32: %.3g; largest |value| %.3g)"
              % (name, field, np.abs(got - want64).max(), np.abs(want32 - want64).max(), np.abs(want64).max()))
        U.assert_close_fp32(got, want32, want64, RTOL, ATOL, "%s %s" % (name, field))
    assert np.array_equal(mk.n_groups.cpu().numpy(), r64["n_groups"]) and np.array_equal(mk.reached.cpu().numpy(), r64["reached"])
    assert (r64["scale"] > 0).any() and np.abs(r64["deviation"]).max() > 1e-3 and np.abs(r64["group_grad"]).max() > 1e-3


@pytest.mark.parametrize("name", ["e300_L3", "e60_L2"])
def test_relation_tie_and_the_same_tie_as_labels(name):
    from red_gnn_amd import explain
    c, model, rd, e = _setup(name)
    mk = _mask(name, "relation")
    free, fixed = _parts(rd, c.n_rel)
    T = explain.mask_groups(rd, "relation", free)
    ref = TR.groups(e, c.n_rel, "relation", free.cpu().numpy())
    assert np.array_equal(mk.group.cpu().numpy(), ref.group_of) and np.array_equal(mk.group_key.cpu().numpy(), ref.group_key)
    assert int(mk.n_groups.sum()) == ref.n_groups < int(free.sum())
    first, group = _first_member(T), mk.group[free]
    for k in range(len(LAMBDAS)):                                             # one gate per (row, hop, rel)
        assert torch.equal(mk.replica_gate[k][free], mk.replica_gate[k][first][group])
    hop_rel = rd.edges[:, 1].long() * 1000 + rd.edges[:, 3].long()
    per_row = torch.stack([rd.edges[:, 0].long(), hop_rel, mk.gate.view(torch.int32).long()], 1)[free]
    assert torch.unique(per_row, dim=0).shape[0] == ref.n_groups              # (the same condition, stated without mask_groups)
    assert mk.format_groups(k=1)[0].startswith("row 0: hop")
    # ---- labels carrying (hop, rel) in one number: the same groups in the same order, so the same bits
    label = rd.edges[:, 1].long() * (2 * c.n_rel + 1) + rd.edges[:, 3].long()
    lb = rd.learn_tied_mask(model, tie=label, **KW)
    assert torch.equal(lb.group, mk.group) and torch.equal(lb.replica_gate, mk.replica_gate) and torch.equal(lb.group_gate, mk.group_gate)
    for field in ("gate", "keep", "score", "hard_score", "kept_score", "size", "replica"):
        assert torch.equal(getattr(lb, field), getattr(mk, field)), field
    assert lb.group_key.shape[1] == 1 and torch.equal(lb.group_key[:, 0], mk.group_key[:, 0] * (2 * c.n_rel + 1) + mk.group_key[:, 1])
    by_numpy = rd.learn_tied_mask(model, tie=label.cpu().numpy(), **KW)
    assert torch.equal(by_numpy.replica_gate, mk.replica_gate)


@pytest.mark.parametrize("name", list(R.CASES))
def test_rows_cut_off_by_keep_only_decay(name):
    c, model, rd, e = _setup(name)
    keep = ~rd.fact_mask(c.facts, rows=c.fact_rows)
    mk = rd.learn_tied_mask(model, tie="fact", lambdas=(0.5,), iterations=5, lr=0.3, theta0=1.0, keep=keep)
    free, fixed = _parts(rd, c.n_rel, keep)
    gone = ~mk.reached
    assert bool(gone.any()) and 4 * int(mk.reached.sum()) >= c.B
    gone_e = gone[rd.edges[:, 0].long()]
    assert bool((free & gone_e).any()) and not mk.keep[free & gone_e].any(), name + ": a free edge of a row that is not reached is kept"
    assert not mk.score[gone].any() and not mk.kept_score[gone].any() and not mk.target[gone].any() and not mk.size[gone].any()
    assert not mk.keep[~keep].any() and not mk.gate[~keep].any() and bool(mk.keep[fixed].all())
    assert bool((mk.group[~free] == -1).all()) and bool((mk.group[free] >= 0).all())            # only the free edges are tied
    assert not mk.group_gate[gone[mk.group_row]].gt(0.5).any()
    assert torch.equal(mk.kept_score, rd.rescore(model, keep=mk.keep).score)
    assert torch.equal(mk.reached, rd.rescore(model, keep=keep).reached)


def test_model_learn_mask_is_explain_then_the_digraph_call():
    c, model, rd, e = _setup("e60_L3")
    kw = dict(lambdas=(0.1, 0.4), iterations=2, lr=0.2)
    a, b = model.learn_mask(c.subs, c.rels, c.objs, tie="fact", **kw), model.explain(c.subs, c.rels, c.objs).learn_tied_mask(model, tie="fact", **kw)
    for field in ("gate", "keep", "score", "hard_score", "kept_score", "target", "baseline_score", "size", "n_free", "replica", "reached", "live",
                  "group", "group_row", "group_key", "group_gate", "n_groups"):
        assert torch.equal(getattr(a, field), getattr(b, field)), field
    assert torch.equal(a.digraph.edges, rd.edges) and a.tie == "fact" and int(a.n_groups.sum()) < int(a.n_free.sum())
    untied = model.learn_mask(c.subs, c.rels, c.objs, **kw)                   # tie=None: today's path
    assert untied.tie is None and untied.group_gate is None and torch.equal(untied.gate, rd.learn_mask(model, **kw).gate)
    for p in model.parameters():
        assert p.grad is None                                 # the parameters are constants of the mask


def test_learn_tied_mask_inductive():
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    mode = "inductive"
    fx, ids = U.load("ind_WN18RR_v1_%s.npz" % mode), U.load("ind_WN18RR_v1_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    model = RED_GNN_induc(P(n_layer, d, a, loader.n_rel, str(fx["act"])), loader).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    subs, rels = fx["subs"].astype(np.int64)[:12], fx["rels"].astype(np.int64)[:12]
    rd = model.explain(subs, rels, mode=mode)
    kw = dict(lambdas=(0.05, 0.5), iterations=2, lr=0.2)
    mk = rd.learn_tied_mask(model, tie="fact", mode=mode, **kw)
    assert torch.equal(mk.kept_score, rd.rescore(model, keep=mk.keep, mode=mode).score)
    assert torch.equal(mk.target, rd.rescore(model, mode=mode).score)
    free, fixed = _parts(rd, rd.n_rel)
    sel = mk.group_gate > 0.5
    assert torch.equal(mk.keep, rd.fact_mask(mk.group_key[sel], rows=mk.group_row[sel]) | fixed)
    assert torch.equal(mk.gate[free], mk.group_gate[mk.group[free]])
    one = rd.learn_tied_mask(model, tie="fact", mode=mode, **dict(kw, lambdas=(0.5,)))
    assert torch.equal(one.gate, mk.replica_gate[1])
    by_model = model.learn_mask(subs, rels, mode=mode, tie="fact", **kw)
    assert torch.equal(by_model.gate, mk.gate) and torch.equal(by_model.digraph.edges, rd.edges)
