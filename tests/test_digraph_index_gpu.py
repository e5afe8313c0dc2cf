"""engine.digraph_hop_ranges / digraph_hop_index (rg_digraph_hop_ranges, rg_digraph_hop_index; csrc/digraph_index.hip) on the MI355X
(-m gpu): exact-equal against the numpy statement tests/digraph_index_ref.py and against explain._hop_index, the torch build the
static and interpolation drivers keep, on hand-made digraphs and on hops whose sizes straddle the wave (64), block (256) and
scan-tile (2048) boundaries.  Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import digraph_index_ref as IR

pytestmark = pytest.mark.gpu

N_ENT, N_ROWS_TAB = 10, 3
HAND = np.array([[0, 1, 3, 0, 3], [0, 1, 3, 1, 4], [0, 1, 3, 2, 4], [0, 2, 3, 0, 7], [0, 2, 4, 1, 7], [0, 2, 5, 1, 7],
                 [1, 1, 6, 0, 4], [1, 2, 4, 2, 4], [1, 2, 4, 0, 4]])         # test_xrescore_ref's: row 0 ends at node 4, row 1 starts there
HAND_SUBS = [3, 6]


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def _offsets(edges, B):
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(np.asarray(edges, np.int64).reshape(-1, 5)[:, 0], minlength=B))
    return off


def _walk(edges, B, L, subs, n_ent=N_ENT, n_rows=N_ROWS_TAB, keep=None, time=None, live_fill=5, check=True):
    """Every hop through the engine, chained through ``keys``; with ``check`` each hop's arrays are compared with the numpy reference
    and with explain._hop_index.  Returns (the hops' tuples, live uint8 [E] on the host).  A non-zero status raises the driver's error."""
    from red_gnn_amd import engine, explain
    edges = np.asarray(edges, np.int64).reshape(-1, 5)
    off = _offsets(edges, B)
    E = len(edges)
    e_d, off_d = _dev(edges, torch.int32), _dev(off, torch.int64)
    keep_d = None if keep is None else _dev(np.asarray(keep).astype(np.uint8), torch.uint8)
    time_d = None if time is None else _dev(time, torch.int32)
    live = torch.full((E,), live_fill, dtype=torch.uint8, device="cuda")
    ranges = engine.digraph_hop_ranges(e_d, off_d, L)
    if ranges.status:
        raise engine.digraph_index_error(ranges.status, "rescore", L, n_ent, n_rows)
    if check:
        assert np.array_equal(ranges.hop_ptr.cpu().numpy(), IR.hop_ranges(edges, off, L)) and np.array_equal(ranges.hop_ptr_host, IR.hop_ranges(edges, off, L))
        assert ranges.hop_edges == [int((edges[:, 1] == l).sum()) for l in range(1, L + 1)]
    e64 = e_d.long()
    row, hop, head, _, tail = e64.unbind(1)
    kept = torch.ones(E, dtype=torch.bool, device="cuda") if keep_d is None else keep_d.bool()
    keys_prev = torch.arange(B, device="cuda") * n_ent + _dev(subs, torch.int64)
    live_t = torch.zeros(E, dtype=torch.bool, device="cuda")
    hops = []
    for l in range(1, L + 1):
        got = engine.digraph_hop_index(e_d, ranges, l, keys_prev, n_ent, n_rows, live, keep_d, time_d)
        if got[-1]:
            raise engine.digraph_index_error(got[-1], "rescore", L, n_ent, n_rows)
        at, src, rel, tm, keys, dst_ptr, row_of, prev_idx, _ = got
        hops.append(got)
        if check:
            ref = IR.hop_index(edges, off, l, L, keys_prev.cpu().numpy(), n_ent, n_rows, None if keep is None else np.asarray(keep).astype(bool), time)
            for name, x in (("at", at), ("src", src), ("rel", rel), ("keys", keys), ("dst_ptr", dst_ptr), ("row_of", row_of), ("prev_idx", prev_idx)):
                assert x.dtype == (torch.int64 if name == "keys" else torch.int32), name
                assert np.array_equal(x.cpu().numpy(), ref[name]), (l, name, x.cpu().numpy(), ref[name])
            assert (tm is None) == (time is None) and (tm is None or np.array_equal(tm.cpu().numpy(), ref["time"]))
            torch_at = torch.nonzero((hop == l) & kept).reshape(-1)
            old = explain._hop_index("rescore", l, L, torch_at, row, head, tail, keys_prev, n_ent, live_t)
            if old is None:
                assert at.numel() == 0 and keys.numel() == 0 and dst_ptr.numel() == 0
            else:
                o_at, o_src, o_keys, o_ptr, o_row, o_prev, _ = old
                assert torch.equal(at.long(), o_at) and torch.equal(src.long(), o_src) and torch.equal(keys, o_keys)
                assert torch.equal(dst_ptr, o_ptr) and torch.equal(row_of.long(), o_row) and torch.equal(prev_idx, o_prev)
                assert torch.equal(rel.long(), e64[o_at, 3])
        if at.numel() == 0:
            break
        keys_prev = keys
    live_h = live.cpu().numpy()
    if check:
        assert np.array_equal(live_h == 1, live_t.cpu().numpy()) and (live_h[live_h != 1] == live_fill).all()     # untouched elsewhere
    return hops, live_h


def test_hand_made_digraphs():
    time = np.arange(9) + 20
    hops, live = _walk(HAND, 2, 2, HAND_SUBS, time=time)
    assert hops[0][4].tolist() == [3, 4, 14] and hops[0][5].tolist() == [0, 1, 3, 4]      # node 4 of row 0 and of row 1: two nodes
    assert hops[1][4].tolist() == [7, 14] and hops[1][0].tolist() == [3, 4, 7, 8] and hops[1][7].tolist() == [-1, 2]
    assert hops[0][3].tolist() == [20, 21, 22, 26] and live.tolist() == [1, 1, 1, 1, 1, 5, 1, 1, 1]
    for keep in (np.ones(9, bool), np.zeros(9, bool), np.arange(9) % 2 == 0, np.array([1, 0, 0, 1, 1, 1, 1, 1, 0], bool), None):
        _walk(HAND, 2, 2, HAND_SUBS, keep=keep, time=time)
        _walk(HAND, 2, 2, HAND_SUBS, keep=keep)
    # a hop without kept edges: the walk ends there, hop 2 is never asked for
    hops, live = _walk(HAND, 2, 2, HAND_SUBS, keep=HAND[:, 1] == 2)
    assert len(hops) == 1 and hops[0][0].numel() == 0 and (live == 5).all()
    # E = 0
    hops, live = _walk(np.zeros((0, 5), np.int64), 2, 2, [3, 6])
    assert len(hops) == 1 and hops[0][0].numel() == 0 and live.size == 0
    # a row without edges: first, middle and last
    for empty in (0, 1, 2):
        rows = [b for b in range(3) if b != empty]
        e = HAND.copy()
        e[:, 0] = np.array(rows)[e[:, 0]]
        subs = [0, 0, 0]
        subs[rows[0]], subs[rows[1]] = HAND_SUBS
        hops, _ = _walk(e, 3, 2, subs)
        assert hops[1][6].tolist() == rows                                               # hop L: one destination per row that has one
    # B = 1, L = 1
    hops, live = _walk([[0, 1, 3, 0, 5], [0, 1, 3, 2, 5]], 1, 1, [3])
    assert hops[0][4].tolist() == [5] and hops[0][5].tolist() == [0, 2] and live.tolist() == [1, 1]


def _big(n_hop, n_ent=8000):
    """Two rows, three hops.  Hop 2 has ``n_hop`` edges, row 0's in runs of 1, 128, 129 and 300 edges into one destination (then
    single edges), fed by hop 1's fan-out from s = 0; hop 3 leads every hop-2 node to the answer 7999.  Row 1 is three edges."""
    runs, left = [], n_hop - 1                                         # (row 1 brings the hop's last edge)
    for r in [1, 128, 129, 300] + [1] * n_hop:
        if left == 0:
            break
        runs.append(min(r, left))
        left -= runs[-1]
    heads = np.arange(1, 301)                                           # hop 1: s -> 1..300
    e = [[0, 1, 0, 0, int(h)] for h in heads]
    tails = 1000 + np.arange(len(runs))
    for t, r in zip(tails, runs):                                       # hop 2: the first r heads -> t
        e += [[0, 2, int(h), int(h) % 3, int(t)] for h in heads[:r]]
    e += [[0, 3, int(t), 1, n_ent - 1] for t in tails]
    e += [[1, 1, 7, 0, 8], [1, 2, 8, 1, 9], [1, 3, 9, 2, 9]]
    return np.array(e, np.int64), runs


@pytest.mark.parametrize("n_hop", [63, 64, 65, 255, 256, 257, 1025, 2047, 2048, 2049, 4100])
def test_hops_across_wave_block_and_scan_tile_boundaries(n_hop):
    from red_gnn_amd import engine
    edges, runs = _big(n_hop)
    assert (edges[:, 1] == 2).sum() == n_hop and sum(runs) == n_hop - 1 and runs[0] == 1
    time = (np.arange(len(edges)) * 7) % 50
    for keep in (None, np.arange(len(edges)) % 2 == 0, np.arange(len(edges)) % 3 != 1):
        hops, live = _walk(edges, 2, 3, [0, 7], n_ent=8000, keep=keep, time=time)
        if keep is None:
            ptr = hops[1][5].cpu().numpy()
            assert np.diff(ptr).tolist() == runs + [1]                            # dst_ptr feeds rg_digraph_tlayer_fwd's cut
            assert engine.digraph_chunks(ptr)[0] == sum(r > engine.DIGRAPH_CHUNK for r in runs)
            assert (live == 1).all()
    # two runs give identical bits
    a, la = _walk(edges, 2, 3, [0, 7], n_ent=8000, keep=np.arange(len(edges)) % 3 != 1, time=time, check=False)
    b, lb = _walk(edges, 2, 3, [0, 7], n_ent=8000, keep=np.arange(len(edges)) % 3 != 1, time=time, check=False)
    assert np.array_equal(la, lb) and len(a) == len(b)
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x[:-1], y[:-1]))


def test_a_hop_with_hop_edges_only_in_the_second_row_and_live_over_hops():
    """Row 0 is one hop-1 edge that leads nowhere, row 1 carries everything: the rows' segments of a hop are not adjacent."""
    e = np.array([[0, 1, 2, 0, 3], [1, 1, 6, 0, 4], [1, 1, 6, 1, 5], [1, 2, 4, 2, 9], [1, 2, 5, 0, 9]])
    hops, live = _walk(e, 2, 2, [2, 6])
    assert hops[1][0].tolist() == [3, 4] and hops[1][6].tolist() == [1] and live.tolist() == [1, 1, 1, 1, 1]


@pytest.mark.parametrize("col,row,value,text", [(4, 2, 2, r"ordered by \(row, hop, tail\)"), (4, 3, 6, "must share their tail"),
                                                (2, 0, N_ENT, "head or tail out of range"), (4, 8, N_ENT, "head or tail out of range"),
                                                (3, 1, N_ROWS_TAB, "relation out of range"), (0, 6, 0, "not the row of its range"),
                                                (1, 1, 2, "not the row of its range"), (1, 0, 0, "not the row of its range"),
                                                (2, 4, -1, "head or tail out of range"), (3, 4, -1, "relation out of range")])
def test_malformed_digraphs_are_refused_not_followed(col, row, value, text):
    bad = HAND.copy()
    bad[row, col] = value
    off = _offsets(HAND, 2)                                             # (the rows' ranges are the well-formed digraph's)
    with pytest.raises(ValueError, match=text):
        from red_gnn_amd import engine
        e_d, off_d = _dev(bad, torch.int32), _dev(off, torch.int64)
        live = torch.zeros(9, dtype=torch.uint8, device="cuda")
        ranges = engine.digraph_hop_ranges(e_d, off_d, 2)
        status, keys_prev = ranges.status, torch.arange(2, device="cuda") * N_ENT + _dev(HAND_SUBS, torch.int64)
        for l in (1, 2):
            if status:
                break
            got = engine.digraph_hop_index(e_d, ranges, l, keys_prev, N_ENT, N_ROWS_TAB, live, None, None)
            status, keys_prev = got[-1], got[4]
        torch.cuda.synchronize()
        raise engine.digraph_index_error(status, "rescore", 2, N_ENT, N_ROWS_TAB)


def test_wrapper_argument_checks():
    from red_gnn_amd import engine
    e_d, off_d = _dev(HAND, torch.int32), _dev(_offsets(HAND, 2), torch.int64)
    ranges = engine.digraph_hop_ranges(e_d, off_d, 2)
    keys = torch.arange(2, device="cuda") * N_ENT + _dev(HAND_SUBS, torch.int64)
    live = torch.zeros(9, dtype=torch.uint8, device="cuda")
    ok = dict(edges=e_d, ranges=ranges, hop=1, keys_prev=keys, n_ent=N_ENT, n_rela_rows=N_ROWS_TAB, live=live)
    for kw, text in ((dict(edges=e_d.long()), "edges must be int32"), (dict(hop=0), "hop must be"), (dict(hop=3), "hop must be"),
                     (dict(keys_prev=keys.int()), "keys_prev must be an int64"), (dict(live=live.bool()), "live must be uint8"),
                     (dict(live=live[:8]), "live must be uint8"), (dict(keep=live.bool()), "keep must be uint8"),
                     (dict(edge_time=keys), "edge_time must be int32"), (dict(n_ent=0), "n_ent must be"), (dict(ranges=None), "ranges must be"),
                     (dict(edges=e_d.cpu()), "on one device|MI355X")):
        with pytest.raises((ValueError, RuntimeError), match=text):
            engine.digraph_hop_index(**{**ok, **kw})
    for kw, text in ((dict(edges=e_d.long()), "edges must be int32"), (dict(offsets=off_d.int()), "offsets must be int64"), (dict(n_hops=0), "n_hops"),
                     (dict(n_hops=33), "n_hops")):
        with pytest.raises(ValueError, match=text):
            engine.digraph_hop_ranges(**{**dict(edges=e_d, offsets=off_d, n_hops=2), **kw})
