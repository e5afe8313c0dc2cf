"""rg_layer_fwd as captured inference runs it (models._GraphedInference: reset, then per hop expand_nodes_async -> layer_fwd_into), and
the word-parallel walk with tickets of more than one item.  After an asynchronous expansion the host knows no size: n_new is a hint that
alone picks the dense or the filter flavour of the per-query walk, the word-parallel walk bounds the previous level by B * n_ent rows and
sizes its tickets from the caller's edge hint (or nothing), the first walk after an expansion launches no zeroing kernel (queues_clean),
and a captured sequence is replayed on frontiers of other sizes than the recorded ones with every buffer as the last replay left it.

Conventions of every test: agg is pre-filled with NaN and has 300 guard rows past the level's count, which must still be NaN afterwards;
hidden and a_s carry 300 more rows of NaN, so a read past the previous level's count shows as NaN in agg; the scratch (partial rows and
their `written` bytes) starts as 0xFF bytes - flags set, partial rows NaN - so a launch that relied on what an earlier one left shows
too.  Rows [0, n_new) are checked against layer_ref.forward in fp64 with layer_ref.bound(S, n, n0, C_BOUND) (nothing new is chosen
here), pad columns must be zero, and every walk must equal the per-query walk of a synchronously expanded frontier bit for bit.

Not covered: the temporal and windowed kernels (the models capture no such sequence), and the fall-back to the per-query walk where
B * n_ent * ld * 4 >= 4 GiB would overflow the word-parallel walk's 32-bit row offsets (rgwp::offsets_fit; a frontier of that size is
no test of a few seconds).  In the captured test `tickets` runs the single-source walk or the per-query walk (what inference records for
a first hop); its word-parallel walks are test 1's and test 2's.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import layer_ref as lr

pytestmark = pytest.mark.gpu

# wall time of this file on an MI355X: 9.6 s (44 tests; the slowest, tickets replayed from every query's hub with 2.1 M edges, 3.8 s: its fp64
# reference, formed once for the three ways to freeze the hints)
KEYS = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")
GUARD = 300
SENTINEL = -7
NAN = float("nan")
STATIC = [name for name, make in lr.CASES.items() if make().kind == "static"]
FRESH = ("default", "b65_e97", "hubs", "tickets")      # every call also as the first launch after an expansion
SETS = ("recorded", "isolated", "hub")


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _prev(old, new, n_ent):
    """Row of every new node in the (sorted) previous level, -1 where it was not there."""
    ko, kn = old[:, 0] * n_ent + old[:, 1], new[:, 0] * n_ent + new[:, 1]
    pos = np.minimum(np.searchsorted(ko, kn), len(ko) - 1)
    return np.where(ko[pos] == kn, pos, -1).astype(np.int32)


def _oracle(name, which="recorded"):
    """(case, per hop: nodes, prev, inputs, fp64 forward; level counts) from the CPU oracle.  ``which``: the case's own start, or every
    query from the isolated entity n_ent - 1 / from the hub entity 3 (_rand_triples: the tail of a tenth of the triples)."""
    case = lr.CASES[name]()
    if which != "recorded":
        case.nodes0 = np.stack([np.arange(case.B), np.full(case.B, case.n_ent - 1 if which == "isolated" else 3)], 1).astype(np.int64)
    hops, counts = [], [(len(case.nodes0), 0)]
    for k, (old, new, _, hop) in enumerate(lr.hops(case)):
        x = lr.inputs(case, k, hop)
        x.pop("grad_agg")
        f64 = lr.forward(hop, *(x[kk] for kk in KEYS))
        hops.append(types.SimpleNamespace(hop=hop, nodes=new.astype(np.int32), prev=_prev(old, new, case.n_ent), x=x, agg=f64.agg,
                                          bound=lr.bound(f64.S["agg"], f64.n["agg"], lr.n0_of("agg", case.d, case.attn_dim), lr.C_BOUND)))
        counts.append((hop.n_new, hop.E))
    return case, hops, counts


def _start(case, fr):
    if case.reset == "subjects":
        fr.reset(_dev(case.nodes0[:, 1], torch.int32))
    else:
        fr.reset_nodes(_dev(case.nodes0, torch.int32))


def _node_buffers(case):
    cap = case.B * case.n_ent
    return (torch.full((cap, 2), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda"))


def _expand_async(fr, g, k, nodes, prev):
    """Hop k + 1 without a read-back: odd hops as expand_async + nodes_into, even hops as the fused expand_nodes_async."""
    if k % 2 == 0:
        fr.expand_async(g)
        fr.nodes_into(nodes, prev)
    else:
        fr.expand_nodes_async(g, nodes, prev)
    assert (fr.n_new, fr.n_edges) == (-1, -1)


def _check_nodes(what, ref, nodes, prev):
    n = ref.hop.n_new
    assert np.array_equal(nodes[:n].cpu().numpy(), ref.nodes), what + ": node list differs from the oracle's"
    assert np.array_equal(prev[:n].cpu().numpy(), ref.prev), what + ": links to the previous level differ from the oracle's"
    assert bool((nodes[n:] == SENTINEL).all()) and bool((prev[n:] == SENTINEL).all()), "%s: rows past N = %d were written" % (what, n)


def _padded_inputs(x, rows=None):
    """Device copies of a hop's inputs; hidden and a_s with GUARD more rows (or ``rows`` rows in all) of NaN."""
    X = {k: _dev(v) for k, v in x.items() if v is not None}
    for k in ("hidden", "a_s"):
        n = X[k].shape[0]
        X[k] = torch.cat([X[k], torch.full(((n + GUARD if rows is None else rows) - n, X[k].shape[1]), NAN, device="cuda")])
    return X


def _scratch(fr, g, ld):
    from red_gnn_amd import engine as eng
    return torch.empty(max(eng.layer_fwd_scratch_bytes(fr, g, ld), 256), dtype=torch.uint8, device="cuda")


def _layer(case, g, fr, X, agg, scratch, n_hint, walk):
    from red_gnn_amd import engine as eng
    eng.layer_fwd_into(fr, g, fr.level, n_hint, X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"],
                       case.attn_dim, agg, scratch, walk=walk)


def _run(case, g, fr, X, scratch, n_new, n_hint, walk):
    """One layer forward into a fresh NaN agg of n_new + GUARD rows, the scratch set to 0xFF bytes first."""
    agg = torch.full((n_new + GUARD, case.ld), NAN, dtype=torch.float32, device="cuda")
    scratch.fill_(0xFF)
    _layer(case, g, fr, X, agg, scratch, n_hint, walk)
    return agg


def _set_hint(fr, hint):
    from red_gnn_amd import _lib
    _lib.check(_lib.lib().rg_frontier_set_edge_hint(fr.handle, -1 if hint is None else int(hint)))


def _check_bound(what, agg, ref, case):
    """Rows [0, n_new) of agg within the fp64 bound, pad columns zero, every row from n_new on still NaN.  Returns the worst ratio."""
    n = ref.hop.n_new
    assert bool(torch.isnan(agg[n:]).all()), what + ": rows past the level's count were written"
    a = agg[:n].cpu().numpy().astype(np.float64)
    assert not np.isnan(a).any(), "%s: %d elements never written, or NaN read from past the previous level" % (what, int(np.isnan(a).sum()))
    err = np.abs(a - ref.agg)
    ok = err <= ref.bound
    # (layer_ref.worst_ratio from the bound: bound = C_BOUND (n + n0) u S + tiny)
    ratio = lr.C_BOUND * float(np.max(np.maximum(err - lr.TINY, 0.0) / np.maximum(ref.bound - lr.TINY, 1e-300), initial=0.0))
    assert ok.all(), "%s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g); first at %s" % (
        what, int((~ok).sum()), ok.size, ratio, lr.C_BOUND, np.argwhere(~ok)[0])
    assert not a[:, case.d:].any(), what + ": pad columns of agg"
    return ratio


def _same(what, agg, A1, n):
    """agg == A1 bit for bit on rows [0, n); NaN from n on."""
    assert bool(torch.isnan(agg[n:]).all()), what + ": rows past the level's count were written"
    if not torch.equal(agg[:n], A1[:n]):
        bad = (agg[:n] != A1[:n]).any(1)
        never = torch.isnan(agg[:n]).any(1)
        raise AssertionError("%s: %d of %d rows differ from the per-query walk of the synchronous frontier (%d of them hold NaN: never "
                             "written); first row %d" % (what, int(bad.sum()), n, int(never.sum()), int(torch.nonzero(bad)[0])))


# ---- 1. the device-count form, eager ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STATIC)
def test_device_count_form_equals_the_synchronous_per_query_walk(name):
    """Hop by hop on a frontier expanded without read-backs: node list, links and level_counts() are the oracle's; then the per-query walk
    in the flavour the hop's size would not pick (n_hint 1: filter; B * n_ent: dense), every word-parallel walk with the edge hint
    unset, 0, the true E and 2^40, and the single-source walk on hop 1 all give the agg of walk 1 on a synchronously expanded frontier
    bit for bit, which is within the fp64 bound.  On one frontier only the first call runs as the first launch after the expansion
    (no zeroing kernel: queues_clean); for the cases of FRESH every call is repeated after a reset and expansion of its own."""
    from red_gnn_amd import _lib, engine as eng
    case, hops, counts = _oracle(name)
    g = eng.Graph(case.n_ent, case.n_rel, case.triples)
    frS, frA = eng.Frontier(case.n_ent, case.B, n_levels=case.hops + 1), eng.Frontier(case.n_ent, case.B)      # (inference keeps two levels)
    _start(case, frS)
    _start(case, frA)
    scratch = _scratch(frA, g, case.ld)
    grid = case.B * case.n_ent
    has_packs = case.n_ent <= (1 << 20) and case.n_rela_rows < (1 << 12)      # graph.hip: word-parallel packs
    nodes, prev = _node_buffers(case)

    def restart(k):
        _start(case, frA)
        for j in range(k + 1):
            _expand_async(frA, g, j, nodes, prev)

    for k, ref in enumerate(hops):
        tag = "%s hop %d" % (name, k + 1)
        n_new, E = ref.hop.n_new, ref.hop.E
        X = _padded_inputs(ref.x)
        assert frS.expand(g)[:2] == (n_new, E), tag
        A1 = _run(case, g, frS, X, scratch, n_new, n_new, 1)
        ratio = _check_bound(tag + " walk 1, synchronous", A1, ref, case)

        nodes.fill_(SENTINEL)
        prev.fill_(SENTINEL)
        _expand_async(frA, g, k, nodes, prev)
        _check_nodes(tag, ref, nodes, prev)
        assert frA.level_counts() == counts[:k + 2], tag + ": level_counts"

        calls = [(1, 1, None), (1, grid, None)]
        if has_packs:
            calls += [(w, grid, h) for w in range(2, 8) for h in (None, 0, E, 1 << 40)]
        else:
            for w in range(2, 8):      # no packs (wide entity or relation ids): the word-parallel walks are refused
                with pytest.raises(_lib.NativeError):
                    _run(case, g, frA, X, scratch, n_new, grid, w)
        if case.reset == "subjects" and k == 0:
            calls.append((8, grid, None))
        for fresh in ((False, True) if name in FRESH else (False,)):
            for walk, n_hint, hint in calls:
                if fresh:
                    restart(k)
                _set_hint(frA, hint)
                agg = _run(case, g, frA, X, scratch, n_new, n_hint, walk)
                _same("%s walk %d n_hint %d edge hint %s%s" % (tag, walk, n_hint, hint, ", first after an expansion" if fresh else ""),
                      agg, A1, n_new)
        print("%s (n_old %d, n_new %d, E %d): %d calls equal walk 1, agg=%.3g" % (tag, ref.hop.n_old, n_new, E,
                                                                               len(calls) * (2 if name in FRESH else 1), ratio))
    for o in (frS, frA, g):
        o.close()


# ---- 2. tickets of more than one item ---------------------------------------------------------------------------------------------------
TICKET_SIZES = (1, 2, 3, 5, 7, 13, 19, 32)


@pytest.mark.parametrize("name", ["tickets", "tickets_d48"])
def test_word_parallel_tickets_of_every_size_give_the_same_sums(name):
    """The edge hint 200 * n_items // t asks rg_layer_fwd for t items per ticket (layer_fwd.hip wp_tickets; rg_layer_fwd_wp_tickets
    tells what a call gets): walks 3 .. 7 reach 1, 2, 3, 5, 7, 13, 19 and the cap of 32 between them, at least three of which do not
    divide a queue's n_items / 8 items, so that its last ticket is a partial one (layer_fwd_wp.hip resolve).  Each agg equals walk 1's
    bit for bit.  Then the synchronously expanded frontier, whose true edge count sizes the tickets (> 1 on walks 3 .. 7)."""
    from red_gnn_amd import engine as eng
    case, hops, counts = _oracle(name)
    ref = hops[0]
    n_new, E = ref.hop.n_new, ref.hop.E
    g = eng.Graph(case.n_ent, case.n_rel, case.triples)
    frS, frA = eng.Frontier(case.n_ent, case.B), eng.Frontier(case.n_ent, case.B)
    scratch = _scratch(frA, g, case.ld)
    X = _padded_inputs(ref.x)
    _start(case, frS)
    assert frS.expand(g)[:2] == (n_new, E)
    A1 = _run(case, g, frS, X, scratch, n_new, n_new, 1)
    _check_bound(name + " walk 1", A1, ref, case)
    _start(case, frA)
    frA.expand_async(g)
    assert eng.layer_fwd_wp_tickets(frA, g, 1, 1) == (0, 0) and eng.layer_fwd_wp_tickets(frA, g, 1, 8) == (0, 0)

    reached, partial, wrong = set(), set(), []
    n_packs = len(g.export_packs()[2])
    for walk in range(3, 8):
        _, n_items = eng.layer_fwd_wp_tickets(frA, g, 1, walk)
        assert n_items == ((case.B + 31) // 32) * (1 << (walk - 2)) * n_packs and n_items % 8 == 0      # eight queues of n_items / 8 items
        for t in TICKET_SIZES:
            if t > min(n_items // 8192, 32):
                continue
            _set_hint(frA, 200 * n_items // t)
            got, _ = eng.layer_fwd_wp_tickets(frA, g, 1, walk)
            assert got == t, (walk, t, got)
            agg = _run(case, g, frA, X, scratch, n_new, case.B * case.n_ent, walk)
            reached.add(got)
            if (n_items // 8) % got:
                partial.add(got)
            try:
                _same("%s walk %d, %d items per ticket (%d items per queue)" % (name, walk, got, n_items // 8), agg, A1, n_new)
            except AssertionError as exc:
                wrong.append(str(exc))
    assert not wrong, "\n".join(wrong)
    assert reached == set(TICKET_SIZES), sorted(reached)
    assert len(partial) >= 3, "ticket sizes with a partial tail ticket: %s" % sorted(partial)
    print("%s: ticket sizes %s, with a partial tail ticket %s" % (name, sorted(reached), sorted(partial)))

    sizes = {}
    for walk in range(3, 8):      # the true edge count of the synchronous frontier picks the size
        sizes[walk], n_items = eng.layer_fwd_wp_tickets(frS, g, 1, walk)
        assert sizes[walk] > 1, (walk, sizes[walk], n_items)
        agg = _run(case, g, frS, X, scratch, n_new, n_new, walk)
        _same("%s walk %d, synchronous, %d items per ticket" % (name, walk, sizes[walk]), agg, A1, n_new)
    print("%s: ticket sizes from the true E = %d: %s" % (name, E, sizes))
    for o in (frS, frA, g):
        o.close()


# ---- 3. captured and replayed -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    """The oracle hops of (case, subject set), formed once for the three ways to freeze the hints; dropped when the module is done."""
    cache = {}

    def get(name, which):
        if (name, which) not in cache:
            cache[(name, which)] = _oracle(name, which)
        return cache[(name, which)]
    yield get
    cache.clear()


def _eager(case, g, fr, sub, then):
    """The case's hops from the subjects ``sub`` on ``fr``, expanded synchronously; then(k, n_old, n_new, E) after every hop."""
    fr.reset(sub)
    for k in range(case.hops):
        n_new, n_e, n_old = fr.expand(g)
        then(k, n_old, n_new, n_e)


@pytest.mark.parametrize("hints", ["recorded", "default", "isolated"])
@pytest.mark.parametrize("name", ["default", "b33_e1000", "tickets"])
def test_captured_sequence_replayed_on_other_frontiers(name, hints, oracles):
    """reset -> per hop expand_nodes_async + layer_fwd_into, captured once the way models._GraphedInference does (warm-up on a side
    stream, one capture stream, no memset node) with the walk, n_hint and edge hint frozen - as an eager run of the recorded subjects
    gives them (engine.layer_fwd_walk), as the default (B * n_ent, 1, None), or as an eager run of the all-isolated subjects gives them -
    and replayed on: the recorded subjects, every query from the isolated entity, every query from the hub, isolated again, recorded again
    (default, hop 2: 4832 -> 33 -> 6567 -> 33 -> 4832 rows of a grid of 6600).  The inputs are static buffers refilled outside the graph
    (hidden and a_s: NaN past the previous level's count; agg: NaN), everything else is as the previous replay left it.  After every
    replay: level_counts(), node list and links are the oracle's, agg is within the fp64 bound and equals an eager synchronous walk 1 of
    the same subjects bit for bit, and no row past the level's count was written.  b33_e1000: 1056 frontier words, the node list is a
    launch of its own; tickets: 16384 words, the general level build."""
    from red_gnn_amd import _lib, engine as eng
    refs = {which: oracles(name, which) for which in SETS}
    case = refs["recorded"][0]
    n_hops, grid = case.hops, case.B * case.n_ent
    g = eng.Graph(case.n_ent, case.n_rel, case.triples)
    fr, frS = eng.Frontier(case.n_ent, case.B), eng.Frontier(case.n_ent, case.B)
    subs = {which: _dev(refs[which][0].nodes0[:, 1], torch.int32) for which in SETS}

    # static buffers, sized for the largest of the three subject sets
    q_sub = torch.zeros(case.B, dtype=torch.int32, device="cuda")
    rows_old = [max(refs[w][1][k].hop.n_old for w in SETS) + GUARD for k in range(n_hops)]
    rows_new = [max(refs[w][1][k].hop.n_new for w in SETS) + GUARD for k in range(n_hops)]
    X = [_padded_inputs(refs["recorded"][1][k].x, rows_old[k]) for k in range(n_hops)]
    agg = [torch.full((rows_new[k], case.ld), NAN, dtype=torch.float32, device="cuda") for k in range(n_hops)]
    lists = [_node_buffers(case) for _ in range(n_hops)]
    scratch = _scratch(fr, g, case.ld)
    scratch.fill_(0xFF)
    scratchS = _scratch(frS, g, case.ld)

    def refill(which):
        q_sub.copy_(subs[which])
        for k in range(n_hops):
            ref = refs[which][1][k]
            for key, buf in X[k].items():
                src = _dev(ref.x[key])
                buf[:src.shape[0]].copy_(src)
                if key in ("hidden", "a_s"):
                    buf[src.shape[0]:].fill_(NAN)
            agg[k].fill_(NAN)
            lists[k][0].fill_(SENTINEL)
            lists[k][1].fill_(SENTINEL)

    # the frozen hints: (n_hint, walk, edge hint) per hop
    if hints == "default":
        frozen = [(grid, 1, None)] * n_hops
    else:
        frozen = []
        _eager(case, g, frS, subs[hints], lambda k, n_old, n_new, n_e: frozen.append(
            (n_new, eng.layer_fwd_walk(frS, g, frS.level, n_old, n_new, n_e, case.ld), n_e)))
        assert [(h[0], h[2]) for h in frozen] == refs[hints][2][1:]

    def enqueue():
        fr.reset(q_sub)
        for k in range(n_hops):
            n_hint, walk, e_hint = frozen[k]
            fr.expand_nodes_async(g, lists[k][0], lists[k][1], edge_hint=e_hint)
            _layer(case, g, fr, X[k], agg[k], scratch, n_hint, walk)

    refill("recorded")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():       # a warm-up pass on the capture conditions, then the capture itself
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph), torch.no_grad():
        enqueue()
    assert _lib.lib().rg_hipgraph_fill_nodes(ctypes.c_void_p(graph.raw_cuda_graph())) == 0
    graph.instantiate()

    for step, which in enumerate(("recorded", "isolated", "hub", "isolated", "recorded")):
        tag = "%s, hints %s %s, replay %d (%s)" % (name, hints, frozen, step + 1, which)
        _, hops, counts = refs[which]
        refill(which)
        graph.replay()
        torch.cuda.synchronize()
        assert fr.level_counts() == counts, tag + ": level_counts"
        ratios = []

        def compare(k, n_old, n_new, n_e):
            ref = hops[k]
            assert (n_old, n_new, n_e) == (ref.hop.n_old, ref.hop.n_new, ref.hop.E), tag
            what = "%s hop %d" % (tag, k + 1)
            _check_nodes(what, ref, *lists[k])
            ratios.append(_check_bound(what, agg[k], ref, case))
            A1 = torch.full((n_new + GUARD, case.ld), NAN, dtype=torch.float32, device="cuda")
            _layer(case, g, frS, X[k], A1, scratchS, n_new, 1)
            _same(what, agg[k], A1, n_new)
        _eager(case, g, frS, subs[which], compare)
        print("%s: (N, E) %s agg ratios %s" % (tag, counts[1:], " ".join("%.3g" % r for r in ratios)))
    del graph
    for o in (fr, frS, g):
        o.close()
