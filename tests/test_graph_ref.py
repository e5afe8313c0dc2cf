"""tests/graph_ref.py on the CPU: the reference on two hand-written graphs and a hand-written row pointer with every output typed in,
check_packs on correct packings (typed in, and first-fit / best-fit packings of every case that has packs) and on planted faults, and
the case table of tests/test_graph_gpu.py against what its comments claim, computed by the reference alone."""
import numpy as np
import pytest

from tests import graph_ref as G

# ---- a static graph of six entities, two relations, inverses added --------------------------------------------------------------------
# fact rows  0 (0,0,1)  1 (2,1,1)  2 (0,0,1)  3 (3,0,0)  4 (1,1,4)      the triples; row 2 repeats row 0; entity 5 is isolated
#            5 (1,2,0)  6 (1,3,2)  7 (1,2,0)  8 (0,2,3)  9 (4,3,1)      their inverses (t, r + 2, h)
#           10 (0,4,0) 11 (1,4,1) 12 (2,4,2) 13 (3,4,3) 14 (4,4,4) 15 (5,4,5)
HAND_TRIPLES = [[0, 0, 1], [2, 1, 1], [0, 0, 1], [3, 0, 0], [1, 1, 4]]
HAND = {
    "n_fact": 16, "max_in_deg": 5, "max_out_deg": 5,
    # tail 0: rows 3 5 7 10 | tail 1: rows 0 1 2 9 11 | tail 2: 6 12 | tail 3: 8 13 | tail 4: 4 14 | tail 5: 15
    "in_ptr": [0, 4, 9, 11, 13, 15, 16],
    "in_head_rel": [[3, 0], [1, 2], [1, 2], [0, 4], [0, 0], [2, 1], [0, 0], [4, 3], [1, 4], [1, 3], [2, 4], [0, 2], [3, 4], [1, 1], [4, 4],
                    [5, 4]],
    # head 0: rows 0 2 8 10 | head 1: rows 4 5 7 6 11 (relation 1, 2, 2, 3, 4) | head 2: 1 12 | head 3: 3 13 | head 4: 9 14 | head 5: 15
    "out_ptr": [0, 4, 9, 11, 13, 15, 16],
    "out_rel_tail": [[0, 1], [0, 1], [2, 3], [4, 0], [1, 4], [2, 0], [2, 0], [3, 2], [4, 1], [1, 1], [4, 2], [0, 0], [4, 3], [3, 1], [4, 4],
                     [4, 5]],
    # relation 0: rows 0 2 3 | 1: rows 1 4 | 2: rows 5 7 8 | 3: rows 6 9 | 4: rows 10 .. 15
    "rel_ptr": [0, 3, 5, 8, 10, 16],
    "rel_ht": [[0, 1], [0, 1], [3, 0], [2, 1], [1, 4], [1, 0], [1, 0], [0, 3], [1, 2], [4, 1], [0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [5, 5]],
    # head 0: rows 10 (tail 0, position 3) 0 (1, 4) 2 (1, 6) 8 (3, 11) | head 1: rows 5 (0, 1) 7 (0, 2) 11 (1, 8) 6 (2, 9) 4 (4, 13) | ...
    "out_bt_rel_tail": [[4, 0], [0, 1], [0, 1], [2, 3], [2, 0], [2, 0], [4, 1], [3, 2], [1, 4], [1, 1], [4, 2], [0, 0], [4, 3], [3, 1],
                        [4, 4], [4, 5]],
    "out_bt_pos": [3, 4, 6, 11, 1, 2, 8, 9, 13, 5, 10, 0, 12, 7, 14, 15],
    # in-rows and out-rows both have 4 5 2 2 2 1 entries, the relation rows 3 2 3 2 6: by length descending, ties in row order
    "in_vr_rows": [[1, 4, 5, -1], [0, 0, 4, -1], [2, 9, 2, -1], [3, 11, 2, -1], [4, 13, 2, -1], [5, 15, 1, -1]],
    "out_vr_rows": [[1, 4, 5, -1], [0, 0, 4, -1], [2, 9, 2, -1], [3, 11, 2, -1], [4, 13, 2, -1], [5, 15, 1, -1]],
    "rel_vr_rows": [[4, 10, 6, -1], [0, 0, 3, -1], [2, 5, 3, -1], [1, 3, 2, -1], [3, 8, 2, -1]],
    "in_vr_n": 6, "out_vr_n": 6, "rel_vr_n": 5, "time_vr_n": 0,
}

# ---- a temporal graph: four entities, three relation rows, three time ids; row 1 is excluded (twice) -------------------------------------
# kept rows  a (0,0,1,2)  b (0,0,1,0)  c (1,2,3,2)  d (0,0,1,2)
HAND_QUADS = [[0, 0, 1, 2], [2, 1, 1, 0], [0, 0, 1, 0], [1, 2, 3, 2], [0, 0, 1, 2]]
HAND_EXCLUDE = [1, 1]
HAND_T = {
    "n_fact": 4, "max_in_deg": 3, "max_out_deg": 3,
    "in_ptr": [0, 0, 3, 3, 4], "in_head_rel": [[0, 0], [0, 0], [0, 0], [1, 2]], "in_time": [2, 0, 2, 2],          # tail 1: a b d | tail 3: c
    "out_ptr": [0, 3, 4, 4, 4], "out_rel_tail": [[0, 1], [0, 1], [0, 1], [2, 3]], "out_time": [2, 0, 2, 2],       # head 0: a b d | head 1: c
    "rel_ptr": [0, 3, 3, 4], "rel_ht": [[0, 1], [0, 1], [0, 1], [1, 3]], "rel_tm": [2, 0, 2, 2],                  # relation 0: a b d | 2: c
    "time_ptr": [0, 1, 1, 4], "time_ht": [[0, 1], [0, 1], [1, 3], [0, 1]], "time_rel": [0, 0, 2, 0],              # time 0: b | time 2: a c d
    "in_pk": [0, 0, 0, (2 << 20) | 1], "out_pk": [1, 1, 1, (2 << 20) | 3],
    "in_vr_rows": [[1, 0, 3, -1], [3, 3, 1, -1], [0, 0, 0, -1], [2, 3, 0, -1]],
    "out_vr_rows": [[0, 0, 3, -1], [1, 3, 1, -1], [2, 4, 0, -1], [3, 4, 0, -1]],
    "rel_vr_rows": [[0, 0, 3, -1], [2, 3, 1, -1], [1, 3, 0, -1]],
    "time_vr_rows": [[2, 1, 3, -1], [0, 0, 1, -1], [1, 1, 0, -1]],
    "in_vr_n": 4, "out_vr_n": 4, "rel_vr_n": 3, "time_vr_n": 3,
}

# ---- rows of 0, 130, 128, 3 and 257 entries -----------------------------------------------------------------------------------------------
HAND_PTR = [0, 0, 130, 258, 261, 518]
HAND_VROWS = [[1, 0, 128, 0], [2, 130, 128, -1], [4, 261, 128, 2], [4, 389, 128, 3], [3, 258, 3, -1], [1, 128, 2, 1], [4, 517, 1, 4],
              [0, 0, 0, -1]]
HAND_SPLIT = [[1, 0, 2, 0], [4, 2, 3, 0]]


def _same(ref, hand):
    for k, v in hand.items():
        assert np.array_equal(ref[k], np.asarray(v)) and not isinstance(ref[k], type(None)), k


def test_hand_static_graph():
    ref = G.build(6, 5, *G.static_rows(6, 2, HAND_TRIPLES, True))
    _same(ref, HAND)
    pk = lambda pairs, rel, ent: [(p[rel] << 20) | p[ent] for p in pairs]
    assert ref["in_pk"].dtype == np.uint32 and ref["in_pk"].tolist() == pk(HAND["in_head_rel"], 1, 0)
    assert ref["out_pk"].tolist() == pk(HAND["out_rel_tail"], 0, 1) and ref["out_bt_pk"].tolist() == pk(HAND["out_bt_rel_tail"], 0, 1)
    for d in ("in", "out", "rel"):
        assert ref[d + "_vr_split"].shape == (0, 4) and ref[d + "_vr_n_split"] == 0 and ref[d + "_vr_n_slots"] == 0
    for k in ("in_time", "out_time", "rel_tm", "time_ptr", "time_ht", "time_rel", "time_vr_rows", "time_vr_split"):
        assert ref[k] is None
    # without inverses: rows 5 .. 9 are gone, everything else keeps its order
    no_inv = G.build(6, 5, *G.static_rows(6, 2, HAND_TRIPLES, False))
    assert no_inv["n_fact"] == 11 and no_inv["rel_ptr"].tolist() == [0, 3, 5, 5, 5, 11]
    assert no_inv["in_head_rel"].tolist() == [[3, 0], [0, 4], [0, 0], [2, 1], [0, 0], [1, 4], [2, 4], [3, 4], [1, 1], [4, 4], [5, 4]]


def test_hand_temporal_graph():
    ref = G.build(4, 3, *G.temporal_rows(HAND_QUADS, HAND_EXCLUDE), n_time=3)
    _same(ref, HAND_T)
    assert ref["out_bt_rel_tail"] is None and ref["out_bt_pos"] is None and ref["out_bt_pk"] is None
    assert all(ref[d + "_vr_n_slots"] == 0 and len(ref[d + "_vr_split"]) == 0 for d in ("in", "out", "rel", "time"))
    every = G.build(4, 3, *G.temporal_rows(HAND_QUADS, [4, 0, 1, 2, 3, 3]), n_time=3)
    assert every["n_fact"] == 0 and every["time_ptr"].tolist() == [0, 0, 0, 0] and every["in_vr_rows"].tolist() == [[e, 0, 0, -1] for e in range(4)]


def test_hand_virtual_rows():
    rows, split, n_slots = G.virtual_rows(HAND_PTR)
    assert rows.dtype == split.dtype == np.int32
    assert rows.tolist() == HAND_VROWS and split.tolist() == HAND_SPLIT and n_slots == 5


def test_mismatches_names_what_differs():
    ref = G.build(6, 5, *G.static_rows(6, 2, HAND_TRIPLES, True))
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    got.update(pack_ent=np.zeros((0, 2), np.int32), pack=np.zeros((0, 4), np.int32), pack_rows=np.zeros((0, 2), np.int32))
    assert G.mismatches(got, ref) == []
    got["rel_ht"][7, 1] = 2
    got["in_pk"] = got["in_pk"].astype(np.int64)
    got["out_bt_pk"], got["time_ptr"] = None, np.zeros(1, np.int32)
    got["out_vr_rows"] = got["out_vr_rows"][:-1]
    got["max_in_deg"] = 4
    del got["rel_ptr"]
    got["extra"] = 1
    assert sorted(G.mismatches(got, ref)) == ["extra", "in_pk", "max_in_deg", "out_bt_pk", "out_vr_rows", "rel_ht", "rel_ptr", "time_ptr"]


# ---- packings -----------------------------------------------------------------------------------------------------------------------------
def _place(vrows, policy="best", segments_alone=True):
    """Pack id of every non-empty virtual row, in their order: a segment of a cut row opens a pack of its own, any other row goes
    into the fullest open shared pack it fits ("best") or the oldest ("first"), or opens one.  The rows of one entry at the end of
    the (length-sorted) list are placed in bulk: they fill the open packs in pack order, then packs of 128.
    segments_alone=False (a fault) treats segments as ordinary rows."""
    live = np.asarray(vrows, np.int64)
    live = live[live[:, 2] > 0]
    n_bulk = 0
    if len(live) > 4096:
        while n_bulk < len(live) and live[len(live) - 1 - n_bulk, 2] == 1 and live[len(live) - 1 - n_bulk, 3] < 0:
            n_bulk += 1
    room, shared, pack_of = [], [], []
    for _, _, length, slot in live[:len(live) - n_bulk].tolist():
        if slot >= 0 and segments_alone:
            room.append(G.PACK - length)
            pack_of.append(len(room) - 1)
            continue
        fits = [p for p in shared if room[p] >= length]
        if not fits:
            room.append(G.PACK)
            shared.append(len(room) - 1)
            fits = [len(room) - 1]
        p = min(fits, key=lambda q: room[q]) if policy == "best" else fits[0]
        room[p] -= length
        pack_of.append(p)
    if n_bulk:
        free = np.repeat(np.array(shared, np.int64), [room[p] for p in shared])[:n_bulk]
        fresh = len(room) + np.arange(n_bulk - len(free)) // G.PACK
        pack_of = np.concatenate([np.array(pack_of, np.int64), free, fresh])
    return live, np.asarray(pack_of, np.int64)


def _materialise(live, pack_of, in_pk):
    """(ent, pack, rows) of a placement: the rows of a pack back to back in placement order."""
    P = int(pack_of.max()) + 1 if len(pack_of) else 0
    order = np.argsort(pack_of, kind="stable")
    live, pack_of = live[order], pack_of[order]
    n_rows = np.bincount(pack_of, minlength=P)
    row0 = np.cumsum(n_rows) - n_rows
    ent = np.tile(np.array([[-1, 0]], np.int32), (P * G.PACK, 1))
    begin = np.cumsum(live[:, 2]) - live[:, 2]
    begin = begin - begin[row0][pack_of]
    k = np.arange(len(live)) - row0[pack_of]
    j = np.arange(int(live[:, 2].sum())) - np.repeat(np.cumsum(live[:, 2]) - live[:, 2], live[:, 2])
    at = np.repeat(pack_of * G.PACK + begin, live[:, 2]) + j
    ent[at, 0] = np.asarray(in_pk, np.uint32)[np.repeat(live[:, 1], live[:, 2]) + j].view(np.int32)
    ent[at, 1] = np.repeat(k, live[:, 2])
    pack = np.stack([row0, n_rows, live[row0, 3], live[row0, 0]], 1).astype(np.int32)
    return ent, pack, live[:, [0, 3]].astype(np.int32)


HAND_IN_PK = (np.arange(518) + 1000).astype(np.uint32)


def test_check_packs_accepts_the_hand_packing():
    """HAND_VROWS packed by hand: the five segments alone, row 2 (128 entries) fills a pack, row 3 (3 entries) has one."""
    ent = np.tile(np.array([[-1, 0]], np.int32), (7 * 128, 1))
    for p, (first, length) in enumerate([(0, 128), (130, 128), (261, 128), (389, 128), (258, 3), (128, 2), (517, 1)]):
        ent[p * 128:p * 128 + length, 0] = 1000 + first + np.arange(length)
    pack = [[0, 1, 0, 1], [1, 1, -1, 2], [2, 1, 2, 4], [3, 1, 3, 4], [4, 1, -1, 3], [5, 1, 1, 1], [6, 1, 4, 4]]
    rows = [[1, 0], [2, -1], [4, 2], [4, 3], [3, -1], [1, 1], [4, 4]]
    G.check_packs(HAND_VROWS, HAND_IN_PK, ent, pack, rows)
    got = _materialise(*_place(HAND_VROWS), HAND_IN_PK)                      # ... which is also what the test's own packer makes of them
    assert np.array_equal(got[0], ent) and got[1].tolist() == pack and got[2].tolist() == rows
    G.check_packs(np.zeros((0, 4), np.int32), HAND_IN_PK, np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 2), np.int32))


# rows of 100, 60, 30, 28, 20 and 8 entries and one of 130 cut in two: best fit packs {100, 28} {60, 30, 20, 8}
SMALL_PTR = [0, 100, 160, 190, 218, 238, 246, 376]


def _small():
    vrows, _, _ = G.virtual_rows(SMALL_PTR)
    in_pk = (7 * np.arange(376) + 5).astype(np.uint32)
    return vrows, in_pk


def test_check_packs_accepts_a_shared_packing_and_reads_it_as_typed():
    vrows, in_pk = _small()
    live, pack_of = _place(vrows)
    assert live[:, 2].tolist() == [128, 100, 60, 30, 28, 20, 8, 2] and pack_of.tolist() == [0, 1, 2, 2, 1, 2, 2, 3]
    ent, pack, rows = _materialise(live, pack_of, in_pk)
    assert pack.tolist() == [[0, 1, 0, 6], [1, 2, -1, 0], [3, 4, -1, 1], [7, 1, 1, 6]]
    assert rows.tolist() == [[6, 0], [0, -1], [3, -1], [1, -1], [2, -1], [4, -1], [5, -1], [6, 1]]
    assert ent[256:256 + 118, 1].tolist() == [0] * 60 + [1] * 30 + [2] * 20 + [3] * 8 and ent[256 + 118:384].tolist() == [[-1, 0]] * 10
    assert ent[256 + 60, 0] == 7 * 160 + 5 and ent[128 + 100, 0] == 7 * 190 + 5
    G.check_packs(vrows, in_pk, ent, pack, rows)
    G.check_packs(vrows, in_pk, *_materialise(*_place(vrows, "first"), in_pk))


def test_check_packs_rejects_planted_faults():
    vrows, in_pk = _small()
    good = _materialise(*_place(vrows), in_pk)

    def fault(msg, edit=None, packing=None):
        ent, pack, rows = (a.copy() for a in (packing or good))
        if edit:
            out = edit(ent, pack, rows)
            ent, pack, rows = out if out is not None else (ent, pack, rows)
        with pytest.raises(AssertionError, match=msg):
            G.check_packs(vrows, in_pk, ent, pack, rows)

    def twice(ent, pack, rows):                 # entity 1's row is listed twice, entity 4's not at all
        rows[5] = rows[3]

    def missing(ent, pack, rows):               # the last row of pack 2 is dropped: its entries become padding
        ent[256 + 110:256 + 118] = (-1, 0)
        pack[2, 1] = 3
        pack[3, 0] = 6
        return ent, pack, np.delete(rows, 6, axis=0)

    def row_index(ent, pack, rows):
        ent[256 + 60, 1] = 2

    def entry(ent, pack, rows):
        ent[128 + 3, 0] += 1

    def padding(ent, pack, rows):
        ent[128 * 4 - 1, 0] = 0

    def padding_index(ent, pack, rows):
        ent[128 * 3 - 1, 1] = 1

    def slot(ent, pack, rows):
        pack[3, 2] = -1

    def entity(ent, pack, rows):
        pack[1, 3] = 3

    def running_sum(ent, pack, rows):
        pack[2, 0] = 2

    fault("missing from the packs or placed twice", twice)
    fault("7 pack rows \\(7 listed\\) for 8 non-empty virtual rows", missing)
    fault("does not carry the index of its row", row_index)
    fault("are not its in_pk entries", entry)
    fault("a padding entry is not", padding)
    fault("a padding entry is not", padding_index)
    fault("pack\\[:, 2\\] is not the slot", slot)
    fault("pack\\[:, 3\\] is not the entity", entity)
    fault("exclusive running sum", running_sum)
    # the two-entry segment of the cut row in the shared pack {60, 30, 20, 8}
    fault("a segment of a cut row shares its pack", packing=_materialise(*_place(vrows, segments_alone=False), in_pk))
    # live rows in placement order: 128 (a segment), 100, 60, 30, 28, 20, 8, 2 (a segment)
    live = _place(vrows)[0]
    needless = _materialise(live, np.array([0, 1, 2, 2, 1, 2, 3, 4]), in_pk)   # {100, 28} {60, 30, 20} {8}: one needless pack is
    G.check_packs(vrows, in_pk, *needless)                                      # within the bound (one shared pack of 64 or less) ...
    with pytest.raises(AssertionError, match="two shared packs are filled to 64 or less"):
        G.check_packs(vrows, in_pk, *_materialise(live, np.array([0, 1, 2, 2, 1, 3, 4, 5]), in_pk))      # ... {20} and {8} are not
    with pytest.raises(AssertionError, match="holds more than 128 entries"):
        G.check_packs(vrows, in_pk, *_materialise(live, np.array([0, 1, 1, 2, 2, 2, 2, 3]), in_pk))      # {100, 60}


PACK_CASES = [k for k in G.STATIC_CASES if k != "unpacked"]


@pytest.mark.parametrize("name", PACK_CASES)
def test_correct_packings_of_the_cases_pass_check_packs(name):
    """The bound check_packs sets (at most one shared pack filled to 64 or less) holds for best-fit and for first-fit packings of
    every case's virtual rows, and so do its other conditions."""
    case, ref = G.case_and_ref(name)
    assert G.wants_packs(case)
    for policy in ("best", "first"):
        ent, pack, rows = _materialise(*_place(ref["in_vr_rows"], policy), ref["in_pk"])
        assert len(rows) == ref["in_vr_n"] and int((ent[:, 0] != -1).sum()) == ref["n_fact"]
        G.check_packs(ref["in_vr_rows"], ref["in_pk"], ent, pack, rows)


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
def _lengths(ref, d):
    return set(np.diff(ref[d + "_ptr"]).tolist())


@pytest.mark.parametrize("name", list(G.CASES))
def test_every_case_is_in_range_and_has_the_builders_sizes(name):
    case, ref = G.case_and_ref(name)
    if case.kind == "static":
        t = case.triples
        assert t.shape[1] == 3 and ((t >= 0) & (t < [case.n_ent, case.n_rel if case.add_inverse else 2 * case.n_rel, case.n_ent])).all()
        assert ref["n_fact"] == (2 if case.add_inverse else 1) * len(t) + case.n_ent and case.n_rela_rows == 2 * case.n_rel + 1
    else:
        h, r, t, tm = G.temporal_rows(case.quads, case.exclude)
        assert ref["n_fact"] == len(h)
        for a, n in ((h, case.n_ent), (r, case.n_rela_rows), (t, case.n_ent), (tm, case.n_time)):
            assert len(a) == 0 or (a.min() >= 0 and a.max() < n)
    for d, n in (("in", case.n_ent), ("out", case.n_ent), ("rel", case.n_rela_rows)) + ((("time", case.n_time),) if case.n_time else ()):
        assert len(ref[d + "_ptr"]) == n + 1 and ref[d + "_ptr"][-1] == ref["n_fact"]
        rows = ref[d + "_vr_rows"]
        assert rows[:, 2].sum() == ref["n_fact"] and (np.diff(rows[:, 2]) <= 0).all() and rows[:, 2].max(initial=0) <= G.VROW_MAX
        assert ref[d + "_vr_n_slots"] == int((rows[:, 3] >= 0).sum()) == int(ref[d + "_vr_split"][:, 2].sum())
    assert (ref["in_pk"] is not None) == (case.n_ent <= 1 << 20 and case.n_rela_rows <= 1 << 12)


@pytest.mark.parametrize("name,rel_ids", [("lengths", (0, 1, 2, 3, 5, 6, 7, 8, 19)), ("lengths_inv", (0, 1, 2, 3, 5, 6, 7, 8, 9))])
def test_lengths_cases(name, rel_ids):
    case, ref = G.case_and_ref(name)
    assert case.n_ent == 40 and case.add_inverse == (name == "lengths_inv")
    assert _lengths(ref, "in") >= set(G.LENGTHS) and _lengths(ref, "out") >= set(G.LENGTHS)
    rel_len = np.diff(ref["rel_ptr"])
    assert rel_len[list(rel_ids)].tolist() == list(G.LENGTHS) and rel_len[4] == 0 and rel_len[-1] == 40
    if case.add_inverse:
        assert rel_len[[r + 10 for r in rel_ids]].tolist() == list(G.LENGTHS) and rel_len[14] == 0
    assert len(np.unique(case.triples, axis=0)) < len(case.triples)                                   # parallel edges
    for col in range(3):
        assert (np.diff(case.triples[:, col]) < 0).any() and (np.diff(case.triples[:, col]) > 0).any()   # shuffled rows
    # every kind of virtual row: whole rows of 1 .. 128, rows cut in two (129 .. 256), three (257) and four (385) segments
    for d in ("in", "out", "rel"):
        n_cut = np.bincount(ref[d + "_vr_split"][:, 2], minlength=5)
        assert n_cut[2] >= 3 and n_cut[3] >= 1 and n_cut[4] >= 1 and n_cut[5:].sum() == 0 and ref[d + "_vr_n_split"] == n_cut.sum()


@pytest.mark.parametrize("name,n", [("scan_2048", 2048), ("scan_2049", 2049)])
def test_scan_cases(name, n):
    case, ref = G.case_and_ref(name)
    assert case.n_ent + 1 == n and (n == G.SCAN_TILE or n == G.SCAN_TILE + 1) and len(case.triples) == 6000
    assert ref["max_in_deg"] > G.VROW_MAX and ref["max_out_deg"] > G.VROW_MAX
    assert ref["in_ptr"][case.n_ent] - ref["in_ptr"][case.n_ent - 1] > 1 and ref["out_ptr"][case.n_ent] - ref["out_ptr"][case.n_ent - 1] > G.VROW_MAX


@pytest.mark.parametrize("name,n", [("rel_scan_2048", 2048), ("rel_scan_2050", 2050)])
def test_rel_scan_cases(name, n):
    case, ref = G.case_and_ref(name)
    assert case.n_rela_rows + 1 == n and case.n_ent == 30
    rel_len = np.diff(ref["rel_ptr"])
    assert rel_len[case.n_rel - 1] > 0 and rel_len[2 * case.n_rel - 1] > 0 and rel_len[2 * case.n_rel] == 30
    assert (rel_len == 0).sum() > 0.95 * case.n_rela_rows and ref["rel_vr_n_slots"] == 4 and rel_len[5] > G.VROW_MAX


def test_packed_limit_and_unpacked_cases():
    case, ref = G.case_and_ref("packed_limit")
    top = (1 << 20) - 1
    assert case.n_ent == 1 << 20 and case.n_rela_rows == 4095 and G.wants_packs(case) and ref["in_pk"] is not None
    t = case.triples
    assert (t[:, 0] == top).sum() >= 150 and (t[:, 2] == top).sum() >= 150 and (t[:, 1] == 2046).sum() >= 40
    assert ((t[:, 0] == top) & (t[:, 1] == 2046) & (t[:, 2] == top)).any() and 2000 <= len(t) <= 5000
    assert (ref["in_pk"] != 0xFFFFFFFF).all() and (ref["out_pk"] != 0xFFFFFFFF).all() and ((4093 << 20) | top) in ref["in_pk"]
    assert ref["in_vr_n_slots"] > 0 and ref["out_vr_n_slots"] > 0
    case, ref = G.case_and_ref("unpacked")
    assert case.n_rela_rows == 4097 and not G.wants_packs(case)
    assert ref["in_pk"] is None and ref["out_pk"] is None and ref["out_bt_pk"] is None and ref["out_bt_rel_tail"] is not None
    assert (case.triples[:, 1] == 2047).any() and ref["in_vr_n_slots"] > 0


def test_smallest_cases():
    case, ref = G.case_and_ref("no_triples")
    assert len(case.triples) == 0 and ref["n_fact"] == case.n_ent and ref["max_in_deg"] == 1 and ref["rel_ptr"].tolist() == [0, 0, 0, 0, 0, 37]
    case, ref = G.case_and_ref("single_entity")
    assert case.n_ent == 1 and ref["in_ptr"].tolist() == [0, 4] and ref["out_rel_tail"].tolist() == [[0, 0], [0, 0], [1, 0], [4, 0]]


def test_temporal_cases():
    case, ref = G.case_and_ref("t_lengths")
    want = set(G.LENGTHS) | {0}
    assert all(_lengths(ref, d) == want for d in ("in", "out", "rel", "time"))
    time_len = np.diff(ref["time_ptr"])
    assert time_len[5] == 0 and time_len[case.n_time - 1] > 0 and np.diff(ref["rel_ptr"])[case.n_rela_rows - 1] > 0
    _, first, count = np.unique(case.quads[:, :3], axis=0, return_index=True, return_counts=True)
    i = first[np.argmax(count)]                                        # an (h, r, t) that repeats, at more than one time id
    assert len(set(case.quads[(case.quads[:, :3] == case.quads[i, :3]).all(1), 3].tolist())) > 1
    case, ref = G.case_and_ref("t_packed_limit")
    assert case.n_rela_rows == 4096 and not G.wants_packs(case) and int(ref["in_pk"].max() >> 20) == 4095
    assert np.diff(ref["rel_ptr"])[4095] >= 3


def test_exclusion_cases():
    case, ref = G.case_and_ref("t_excl_dups")
    assert len(np.unique(case.exclude)) < len(case.exclude) and ref["n_fact"] == len(case.quads) - len(np.unique(case.exclude))
    assert 0 in case.exclude and len(case.quads) - 1 in case.exclude and ref["in_vr_n_slots"] > 0
    case, ref = G.case_and_ref("t_excl_empty")
    assert case.exclude is not None and len(case.exclude) == 0 and ref["n_fact"] == len(case.quads)
    case, ref = G.case_and_ref("t_excl_all")
    assert set(case.exclude.tolist()) == set(range(len(case.quads))) and len(case.exclude) > len(case.quads) and ref["n_fact"] == 0
    case, ref = G.case_and_ref("t_excl_bad_row")
    bad = (case.quads < 0).any(1) | (case.quads >= [case.n_ent, case.n_rela_rows, case.n_ent, case.n_time]).any(1)
    assert bad.sum() == 2 and set(np.flatnonzero(bad).tolist()) < set(case.exclude.tolist()) and ref["n_fact"] == len(case.quads) - 3
