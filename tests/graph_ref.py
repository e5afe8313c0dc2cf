"""Reference of the graph builders (rg_graph_create, rg_graph_create_device, rg_tgraph_create, rg_tgraph_create_excluding) in plain
numpy, written from the definitions of include/redgnn.h and csrc/common.h, plus the case table the builder tests share.
TEST INFRASTRUCTURE.

Deliberately another method than the builders: they count and scatter (graph.hip) or radix-sort keys (graph_device.hip); here every
CSR is one stable np.argsort / np.lexsort over the fact rows.  Names are those of engine.Graph.export_all().

    fact rows   static: the triples, then (add_inverse) their inverses (t, r + n_rel, h), then one identity row (e, 2 n_rel, e) per
                entity.  Temporal: the quadruples as given, without the excluded rows (np.delete).
    CSR by tail      in_ptr, in_head_rel = {head, rel}: fact order inside a row            (+ in_time)
    CSR by head      out_ptr, out_rel_tail = {rel, tail}: by relation, then fact order     (+ out_time)
    CSR by relation  rel_ptr, rel_ht = {head, tail}: fact order                            (+ rel_tm)
    CSR by time id   time_ptr, time_ht = {head, tail}, time_rel: fact order                (temporal graphs)
    packed entries   in_pk = rel << 20 | head, out_pk = out_bt_pk = rel << 20 | tail, where n_ent <= 2^20 and n_rela_rows <= 2^12
    out-list by tail out_bt_rel_tail, out_bt_pos: rows by out_ptr, a head's edges by (tail, position in the CSR by tail); pos = that
                     position (static graphs)
    virtual rows     of each CSR: a row of at most 128 entries whole, slot -1; a longer one cut into ceil(len / 128) segments with
                     consecutive slots; {row id, first entry, length, slot}, stably sorted by length descending.  split = {row id,
                     first slot, segments, 0} of the cut rows in row order; n, n_split, n_slots.
    packs            not rebuilt: check_packs() asserts what a correct packing of the CSR-by-tail's virtual rows is.
"""
import functools
import types

import numpy as np

VROW_MAX = 128                 # common.h RG_VROW_MAX
PACK = 128                     # common.h RG_PACK
PACKED_MAX_ENT = 1 << 20       # common.h rg_graph::in_pk: "present when n_ent <= 2^20 and 2*n_rel+1 <= 2^12"
PACKED_MAX_RELA_ROWS = 1 << 12
SCAN_TILE = 2048               # graph.hip SCAN_T * SCAN_ITEMS
PACK_KEYS = ("pack_ent", "pack", "pack_rows")


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def static_rows(n_ent, n_rel, triples, add_inverse):
    """(head, rel, tail) of every fact row of a static graph, in fact-row order."""
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    ent = np.arange(n_ent, dtype=np.int64)
    inv = [t[:, 2], t[:, 1] + n_rel, t[:, 0]] if add_inverse else [t[:0, 0]] * 3
    return (np.concatenate([t[:, 0], inv[0], ent]), np.concatenate([t[:, 1], inv[1], np.full(n_ent, 2 * n_rel)]),
            np.concatenate([t[:, 2], inv[2], ent]))


def temporal_rows(quads, exclude=None):
    """(head, rel, tail, time id) of every kept row of a temporal graph."""
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    if exclude is not None:
        q = np.delete(q, np.asarray(exclude, np.int64).reshape(-1), axis=0)
    return q[:, 0], q[:, 1], q[:, 2], q[:, 3]


def _ptr(key, n_rows):
    return np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_rows))]).astype(np.int32)


def _pairs(a, b, order):
    return np.stack([a, b], 1)[order].astype(np.int32)


def virtual_rows(ptr):
    """(rows int32 [n, 4], split int32 [n_split, 4], n_slots) of the CSR rows ptr delimits."""
    ptr = np.asarray(ptr, np.int64)
    n = len(ptr) - 1
    length = np.diff(ptr)
    cut = length > VROW_MAX
    n_seg = np.where(cut, (length + VROW_MAX - 1) // VROW_MAX, 1)
    n_slot = np.where(cut, n_seg, 0)
    first_slot = np.cumsum(n_slot) - n_slot
    row = np.repeat(np.arange(n), n_seg)
    k = np.arange(len(row)) - np.repeat(np.cumsum(n_seg) - n_seg, n_seg)             # segment number inside its row
    first = ptr[row] + k * VROW_MAX
    seg_len = np.minimum(VROW_MAX, ptr[row + 1] - first)
    slot = np.where(cut[row], first_slot[row] + k, -1)
    rows = np.stack([row, first, seg_len, slot], 1)[np.argsort(-seg_len, kind="stable")]
    split = np.stack([np.flatnonzero(cut), first_slot[cut], n_seg[cut], np.zeros(int(cut.sum()), np.int64)], 1)
    return rows.astype(np.int32), split.astype(np.int32), int(n_slot.sum())


def build(n_ent, n_rela_rows, H, R, T, TM=None, n_time=0):
    """Every array and scalar of the graph over the fact rows (H, R, T[, TM]) under export_all()'s names; None where the graph has none."""
    H, R, T = (np.asarray(a, np.int64) for a in (H, R, T))
    temporal = TM is not None
    n_fact = len(H)
    g = {"n_fact": n_fact}
    by_tail = np.argsort(T, kind="stable")
    by_head = np.lexsort((R, H))                                   # head, then relation, then fact order (lexsort is stable)
    by_rel = np.argsort(R, kind="stable")
    g["in_ptr"], g["in_head_rel"] = _ptr(T, n_ent), _pairs(H, R, by_tail)
    g["out_ptr"], g["out_rel_tail"] = _ptr(H, n_ent), _pairs(R, T, by_head)
    g["rel_ptr"], g["rel_ht"] = _ptr(R, n_rela_rows), _pairs(H, T, by_rel)
    g["max_in_deg"], g["max_out_deg"] = int(np.diff(g["in_ptr"]).max()), int(np.diff(g["out_ptr"]).max())
    for k in ("in_time", "out_time", "rel_tm", "time_ptr", "time_ht", "time_rel", "in_pk", "out_pk", "out_bt_pk", "out_bt_rel_tail",
              "out_bt_pos", "time_vr_rows", "time_vr_split"):
        g[k] = None
    if temporal:
        TM = np.asarray(TM, np.int64)
        by_time = np.argsort(TM, kind="stable")
        g["in_time"], g["out_time"], g["rel_tm"] = (TM[o].astype(np.int32) for o in (by_tail, by_head, by_rel))
        g["time_ptr"], g["time_ht"], g["time_rel"] = _ptr(TM, n_time), _pairs(H, T, by_time), R[by_time].astype(np.int32)
    packed = n_ent <= PACKED_MAX_ENT and n_rela_rows <= PACKED_MAX_RELA_ROWS
    if packed:
        g["in_pk"] = ((R << 20) | H)[by_tail].astype(np.uint32)
        g["out_pk"] = ((R << 20) | T)[by_head].astype(np.uint32)
    if not temporal:
        pos = np.empty(n_fact, np.int64)
        pos[by_tail] = np.arange(n_fact)                           # where the CSR by tail lists each fact row
        by_head_tail = np.lexsort((pos, T, H))
        g["out_bt_rel_tail"], g["out_bt_pos"] = _pairs(R, T, by_head_tail), pos[by_head_tail].astype(np.int32)
        if packed:
            g["out_bt_pk"] = ((R << 20) | T)[by_head_tail].astype(np.uint32)
    for d, ptr in (("in", g["in_ptr"]), ("out", g["out_ptr"]), ("rel", g["rel_ptr"]), ("time", g["time_ptr"])):
        rows, split, n_slots = (None, None, 0) if ptr is None else virtual_rows(ptr)
        g[d + "_vr_rows"], g[d + "_vr_split"] = rows, split
        g[d + "_vr_n"], g[d + "_vr_n_split"], g[d + "_vr_n_slots"] = (0 if rows is None else len(rows)), (0 if split is None else len(split)), n_slots
    return g


def wants_packs(case):
    """graph.hip build_graph: `if (!TIME && !in_pk.empty() && n_rela_rows < (1 << 12))`."""
    return case.kind == "static" and case.n_ent <= PACKED_MAX_ENT and case.n_rela_rows < PACKED_MAX_RELA_ROWS


def reference(case):
    if case.kind == "static":
        return build(case.n_ent, case.n_rela_rows, *static_rows(case.n_ent, case.n_rel, case.triples, case.add_inverse))
    h, r, t, tm = temporal_rows(case.quads, case.exclude)
    return build(case.n_ent, case.n_rela_rows, h, r, t, tm, case.n_time)


def mismatches(got, ref):
    """Names under which an export_all() dict differs from the reference (value, shape, dtype or presence); the packs are not compared."""
    bad = sorted((set(got) - set(PACK_KEYS)) ^ set(ref))
    for k, want in ref.items():
        have = got.get(k)
        if want is None or have is None:
            ok = want is None and have is None
        elif isinstance(want, int):
            ok = isinstance(have, int) and have == want
        else:
            ok = isinstance(have, np.ndarray) and have.dtype == want.dtype and have.shape == want.shape and np.array_equal(have, want)
        if not ok and k not in bad:
            bad.append(k)
    return bad


def check_packs(vrows, in_pk, ent, pack, rows):
    """Assert that (ent [n_packs * 128, 2], pack [n_packs, 4], rows [*, 2]) is a correct packing of the virtual rows ``vrows`` of the
    CSR by tail whose packed entries are ``in_pk`` (common.h rg_packs):
      - pack[:, 0] is the exclusive running sum of pack[:, 1] and the total is the number of non-empty virtual rows;
      - inside a pack the rows lie back to back from entry 0: row k's entries carry row index k and equal in_pk[first:first+len] of
        the virtual row whose (entity, slot) is rows[row0 + k]; every remaining entry is (-1, 0);
      - every non-empty virtual row appears exactly once;
      - a segment of a cut row is alone in its pack and pack[p, 2] is its slot; every other pack has -1 there;
      - pack[p, 3] is the entity of the pack's first row;
      - no pack holds more than 128 entries;
      - at most one shared pack (slot -1) is filled to 64 or less.
    The last one holds for any placement that opens a pack only when the row fits in no open one: of two shared packs filled to 64 or
    less, the later one's first row is at most 64 long and the earlier one had, at that moment as ever after, at least 64 entries
    free.  It catches a placement that opens packs needlessly without pinning which of several fitting packs is chosen."""
    vrows = np.asarray(vrows, np.int64).reshape(-1, 4)
    ent, pack, rows = np.asarray(ent, np.int64), np.asarray(pack, np.int64), np.asarray(rows, np.int64)
    in_pk = np.asarray(in_pk).astype(np.uint32)
    P = len(pack)
    assert ent.shape == (P * PACK, 2) and pack.shape == (P, 4) and rows.ndim == 2 and rows.shape[1] == 2
    live = vrows[vrows[:, 2] > 0]
    assert (pack[:, 1] >= 1).all(), "a pack without rows"
    assert np.array_equal(pack[:, 0], np.cumsum(pack[:, 1]) - pack[:, 1]), "pack[:, 0] is not the exclusive running sum of pack[:, 1]"
    total = int(pack[:, 1].sum())
    assert total == len(live) == len(rows), "%d pack rows (%d listed) for %d non-empty virtual rows" % (total, len(rows), len(live))
    assert (rows[:, 1] >= -1).all() and (rows[:, 0] >= 0).all()
    K = max(int(live[:, 3].max(initial=-1)), int(rows[:, 1].max(initial=-1))) + 2
    vkey, rkey = live[:, 0] * K + live[:, 3] + 1, rows[:, 0] * K + rows[:, 1] + 1           # (entity, slot) names a virtual row
    order = np.argsort(vkey, kind="stable")
    assert len(np.unique(vkey)) == len(vkey)
    assert np.array_equal(np.sort(rkey), vkey[order]), "a virtual row is missing from the packs or placed twice"
    match = order[np.searchsorted(vkey[order], rkey)]
    first, length, slot, entity = live[match, 1], live[match, 2], live[match, 3], live[match, 0]
    assert (first >= 0).all() and (first + length <= len(in_pk)).all()
    p_of = np.repeat(np.arange(P), pack[:, 1])
    k = np.arange(total) - pack[p_of, 0]
    fill = np.bincount(p_of, weights=length, minlength=P).astype(np.int64)
    assert (fill <= PACK).all(), "a pack holds more than %d entries" % PACK
    begin = np.cumsum(length) - length
    in_pack = begin - begin[pack[:, 0]][p_of]                                             # first entry of the row inside its pack
    j = np.arange(int(length.sum())) - np.repeat(begin, length)
    at = np.repeat(p_of * PACK + in_pack, length) + j
    real = np.zeros(P * PACK, bool)
    real[at] = True
    assert np.array_equal(ent[at, 1], np.repeat(k, length)), "an entry does not carry the index of its row inside the pack"
    assert np.array_equal(ent[at, 0], in_pk[np.repeat(first, length) + j].view(np.int32)), "a row's entries are not its in_pk entries"
    assert (ent[~real, 0] == -1).all() and (ent[~real, 1] == 0).all(), "a padding entry is not (-1, 0)"
    assert (pack[p_of[slot >= 0], 1] == 1).all(), "a segment of a cut row shares its pack"
    assert np.array_equal(pack[:, 2], slot[pack[:, 0]]), "pack[:, 2] is not the slot of a cut row's segment / -1 of a shared pack"
    assert np.array_equal(pack[:, 3], entity[pack[:, 0]]), "pack[:, 3] is not the entity of the pack's first row"
    assert int(((pack[:, 2] == -1) & (fill <= PACK // 2)).sum()) <= 1, "two shared packs are filled to %d or less" % (PACK // 2)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 127, 128, 129, 255, 256, 257, 385)     # one entry, two, and one / two / three / four virtual rows around RG_VROW_MAX


def _static(name, n_ent, n_rel, triples, add_inverse=True):
    return types.SimpleNamespace(name=name, kind="static", n_ent=n_ent, n_rel=n_rel, n_rela_rows=2 * n_rel + 1, n_time=0,
                                 triples=np.asarray(triples, np.int64).reshape(-1, 3), add_inverse=add_inverse)


def _temporal(name, n_ent, n_rela_rows, n_time, quads, exclude=None):
    return types.SimpleNamespace(name=name, kind="temporal", n_ent=n_ent, n_rel=0, n_rela_rows=n_rela_rows, n_time=n_time,
                                 quads=np.asarray(quads, np.int64).reshape(-1, 4),
                                 exclude=None if exclude is None else np.asarray(exclude, np.int64).reshape(-1))


def _degree_edges(sources, sinks, degrees):
    """(head, tail) pairs in which sources[i] is a head and sinks[i] a tail exactly degrees[i] times; pairs repeat (parallel edges)."""
    head, tail = np.repeat(sources, degrees), np.repeat(sinks, degrees)
    return head, np.roll(tail, len(tail) // 3)


def _labels(rng, ids, counts):
    return rng.permutation(np.repeat(ids, counts))


def _lengths_case(name, add_inverse, rel_ids):
    """40 entities in a shuffled id order: nine sources whose out-rows, nine sinks whose in-rows have exactly LENGTHS entries with
    their identity row (with inverses both have both), 22 others with nine more triples among them, so that the nine relation ids
    ``rel_ids`` have exactly LENGTHS facts each; relation 4 (and every other id not in rel_ids) has none."""
    rng = np.random.default_rng(40)
    n_ent, n_rel = 40, 10
    ids = rng.permutation(n_ent)
    sources, sinks, others = ids[:9], ids[9:18], ids[18:]
    h, t = _degree_edges(sources, sinks, np.array(LENGTHS) - 1)
    h, t = np.concatenate([h, others[:9]]), np.concatenate([t, others[1:10]])
    trip = np.stack([h, _labels(rng, rel_ids, LENGTHS), t], 1)
    return _static(name, n_ent, n_rel, trip[rng.permutation(len(trip))], add_inverse)


def _scan_case(name, n_ent):
    """6000 random triples over n_ent entities; entity 7 has 200 more in-edges, the highest entity id 150 more out-edges."""
    rng = np.random.default_rng(n_ent)
    m = 6000
    h, t = rng.integers(0, n_ent, m), rng.integers(0, n_ent, m)
    t[:200], h[200:350] = 7, n_ent - 1
    trip = np.stack([h, rng.integers(0, 3, m), t], 1)
    return _static(name, n_ent, 3, trip[rng.permutation(m)])


def _rel_scan_case(name, n_rel):
    """30 entities, 400 triples over 20 of the n_rel relation ids, the highest among them; relation 5 has 150 of them."""
    rng = np.random.default_rng(n_rel)
    m = 400
    used = np.concatenate([rng.choice(n_rel - 1, 19, replace=False), [n_rel - 1]])
    r = used[rng.integers(0, 20, m)]
    r[:150], r[150:153] = 5, n_rel - 1
    trip = np.stack([rng.integers(0, 30, m), r, rng.integers(0, 30, m)], 1)
    return _static(name, 30, n_rel, trip[rng.permutation(m)])


def _packed_limit_case():
    """3000 triples over 2^20 entities and 2047 relations; the highest entity id is the head of 150 and the tail of 150 others, the
    highest relation id labels 40, and (2^20 - 1, 2046, 2^20 - 1) is among them."""
    rng = np.random.default_rng(20)
    n_ent, n_rel, m = 1 << 20, 2047, 3000
    h, r, t = rng.integers(0, n_ent, m), rng.integers(0, n_rel, m), rng.integers(0, n_ent, m)
    h[:150], t[150:300], r[:40] = n_ent - 1, n_ent - 1, n_rel - 1
    t[0] = n_ent - 1
    trip = np.stack([h, r, t], 1)
    return _static("packed_limit", n_ent, n_rel, trip[rng.permutation(m)])


def _unpacked_case():
    rng = np.random.default_rng(2048)
    n_ent, n_rel, m = 60, 2048, 500
    h, r, t = rng.integers(0, n_ent, m), rng.integers(0, n_rel, m), rng.integers(0, n_ent, m)
    t[:140], r[:3] = 11, n_rel - 1
    return _static("unpacked", n_ent, n_rel, np.stack([h, r, t], 1))


def _t_lengths_case():
    """20 entities: nine sources whose out-rows and nine sinks whose in-rows have exactly LENGTHS entries (a source has no in-edge, a sink
    no out-edge, two entities neither), nine of the relation ids 0..10 and nine of the time ids 0..11 with LENGTHS facts each, the
    highest of either among them; relations 4 and 9 and times 5, 9 and 10 have none."""
    rng = np.random.default_rng(41)
    ids = rng.permutation(20)
    h, t = _degree_edges(ids[:9], ids[9:18], np.array(LENGTHS))
    quads = np.stack([h, _labels(rng, (0, 1, 2, 3, 5, 6, 7, 8, 10), LENGTHS), t, _labels(rng, (0, 1, 2, 3, 4, 6, 7, 8, 11), LENGTHS)], 1)
    return _temporal("t_lengths", 20, 11, 12, quads[rng.permutation(len(quads))])


def _t_packed_limit_case():
    rng = np.random.default_rng(4096)
    n_ent, m = 50, 300
    r = np.array([0, 1, 77, 4094, 4095])[rng.integers(0, 5, m)]
    r[:3] = 4095
    h = rng.integers(0, n_ent, m)
    h[:2] = n_ent - 1
    return _temporal("t_packed_limit", n_ent, 4096, 5, np.stack([h, r, rng.integers(0, n_ent, m), rng.integers(0, 5, m)], 1))


def _t_excluding_case(name, which):
    """400 quadruples over 30 entities, 7 relation rows and 6 time ids (entity 3 has 140 in-edges), and an exclusion list."""
    rng = np.random.default_rng(400)
    n_ent, m = 30, 400
    t = rng.integers(0, n_ent, m)
    t[100:240] = 3
    quads = np.stack([rng.integers(0, n_ent, m), rng.integers(0, 7, m), t, rng.integers(0, 6, m)], 1)
    if which == "dups":
        exclude = np.array([5, 5, 17, 399, 0, 17, 150, 151, 5])
    elif which == "empty":
        exclude = np.zeros(0, np.int64)
    elif which == "all":
        exclude = np.concatenate([rng.permutation(m), [0, 399]])
    else:                                           # row 9 names an entity, row 200 a relation and a time id the graph does not have
        quads[9, 0], quads[200, 1], quads[200, 3] = n_ent + 5, 7, 6
        exclude = np.array([200, 9, 33])
    return _temporal(name, n_ent, 7, 6, quads, exclude)


CASES = {
    # ---- graph.hip host_vrows `if (len <= RG_VROW_MAX)` / `(len + RG_VROW_MAX - 1) / RG_VROW_MAX` / `std::min(RG_VROW_MAX, beg + len - b)`
    # and graph_device.hip vrow_count_kernel `const int cut = len > RG_VROW_MAX;`, vrow_emit_kernel `l = min(RG_VROW_MAX, beg + len - b)`:
    # rows of 1, 2, 127 .. 129, 255 .. 257 and 385 entries by tail, by head and by relation; `const int32_t max_rel = add_inverse ? n_rel :
    # 2 * n_rel;`: relation 19 of 10 without inverses; a relation without facts between used ones; parallel edges; shuffled rows
    "lengths": lambda: _lengths_case("lengths", False, (0, 1, 2, 3, 5, 6, 7, 8, 19)),
    # ---- rg_graph_create `if (add_inverse) { H[n + i] = t; R[n + i] = r + n_rel; T[n + i] = h; }` / rows_kernel `else { H[i] = t; R[i] = r
    # + n_rel; T[i] = h; }`: the same lengths with the inverse rows between the triples and the identity rows
    "lengths_inv": lambda: _lengths_case("lengths_inv", True, (0, 1, 2, 3, 5, 6, 7, 8, 9)),
    # ---- graph.hip scan_exclusive `if (nb == 1)` with n = SCAN_TILE: build_ptr scans n_ent + 1 = 2048 counts in one block
    "scan_2048": lambda: _scan_case("scan_2048", 2047),
    # ---- the same line, n = 2049: scan_reduce_kernel, the recursive scan of two block sums, scan_apply_kernel with offsets
    "scan_2049": lambda: _scan_case("scan_2049", 2048),
    # ---- build_ptr(tmp, R, n_fact, n_rela_rows, rel_ptr, s): n_rela_rows + 1 = 2048, one block; build_vrows over mostly empty rows
    "rel_scan_2048": lambda: _rel_scan_case("rel_scan_2048", 1023),
    # ---- the same, n_rela_rows + 1 = 2050: two blocks
    "rel_scan_2050": lambda: _rel_scan_case("rel_scan_2050", 1024),
    # ---- `if (n_ent <= (1 << 20) && n_rela_rows <= (1 << 12))` and `n_rela_rows < (1 << 12)` (graph.hip) / `const bool packed`, `const
    # bool want_packs` (graph_device.hip) at n_ent = 2^20, n_rela_rows = 4095: packed entries and packs, 20 + 12 key bits
    "packed_limit": _packed_limit_case,
    # ---- the same lines at n_rela_rows = 4097: int2 entries only, no packs
    "unpacked": _unpacked_case,
    # ---- rg_graph_create `n == 0`: identity rows only
    "no_triples": lambda: _static("no_triples", 37, 2, np.zeros((0, 3), np.int64)),
    # ---- graph_device.hip `while (((int64_t)1 << ent_bits) < n_ent) ++ent_bits;` with n_ent = 1: one row of four self-loops
    "single_entity": lambda: _static("single_entity", 1, 2, [[0, 0, 0], [0, 1, 0], [0, 0, 0]], add_inverse=False),
    # ---- build_graph `if (TIME)`: time_ptr / time_ht / time_rel / host_vrows(time_ptr, n_time, ..) and rel_tm; rows of 0 entries
    "t_lengths": _t_lengths_case,
    # ---- build_graph `n_rela_rows <= (1 << 12)` at 4096 on a temporal graph: relation 4095 << 20 in the packed entries, no packs
    "t_packed_limit": _t_packed_limit_case,
    # ---- tgraph_create `drop[exclude[k]] = 1;` twice for a row
    "t_excl_dups": lambda: _t_excluding_case("t_excl_dups", "dups"),
    # ---- tgraph_create `std::vector<char> drop(n_exclude ? n : 0, 0);` with n_exclude = 0: rg_tgraph_create's graph
    "t_excl_empty": lambda: _t_excluding_case("t_excl_empty", "empty"),
    # ---- build_graph with n_fact = 0
    "t_excl_all": lambda: _t_excluding_case("t_excl_all", "all"),
    # ---- tgraph_create `if (n_exclude && drop[i]) continue;` ahead of the range check of the row's ids
    "t_excl_bad_row": lambda: _t_excluding_case("t_excl_bad_row", "bad_row"),
}

STATIC_CASES = [k for k in CASES if not k.startswith("t_")]
TEMPORAL_CASES = [k for k in CASES if k.startswith("t_")]


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(case, reference dict) computed once per process; callers must not modify either."""
    case = CASES[name]()
    return case, reference(case)
