"""Plain-numpy statement of the per-hop index of an edited r-digraph (engine.digraph_hop_ranges / digraph_hop_index,
csrc/digraph_index.hip).  TEST INFRASTRUCTURE: loops over rows and edges, nothing taken from the library.

The digraph: ``edges`` int [E, 5] = (row, hop, head, rel, tail) ordered by (row, hop, tail), ``offsets`` int [B + 1].
"""
import numpy as np

ORDER = "edges must be ordered by (row, hop, tail)"
TWO_TAILS = "must share their tail"
ROW_HOP = "a row that is not the row of its range"
ENTITY = "a head or tail out of range"
RELATION = "a relation out of range"


def hop_ranges(edges, offsets, L):
    """hop_ptr int64 [B, L + 1]: entry (b, l - 1) the first edge of row b with hop >= l, entry (b, L) offsets[b + 1]."""
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    B = len(offsets) - 1
    out = np.zeros((B, L + 1), np.int64)
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        for l in range(1, L + 1):
            at = lo
            while at < hi and e[at, 1] < l:
                at += 1
            out[b, l - 1] = at
        out[b, L] = hi
    return out


def hop_index(edges, offsets, l, L, keys_prev, n_ent, n_rela_rows, keep=None, edge_time=None):
    """The index of hop l: dict(at, src, rel, time, keys, dst_ptr, row_of, prev_idx), n_live = len(at), n_dst = len(keys); ``time`` is
    None without ``edge_time``.  An edge is live iff it is kept, has hop l and its (row, head) is in ``keys_prev`` (sorted, unique
    row * n_ent + entity).  ValueError with one of the texts above where the hop's edges are malformed, kept or not."""
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    ptr = hop_ranges(e, offsets, L)
    B = len(offsets) - 1
    where = {int(k): i for i, k in enumerate(np.asarray(keys_prev).tolist())}
    at, src = [], []
    for b in range(B):
        if ptr[b, 0] != offsets[b]:
            raise ValueError(ROW_HOP)
        last = None
        for i in range(int(ptr[b, l - 1]), max(int(ptr[b, l]), int(ptr[b, l - 1]))):
            row, hop, head, rel, tail = e[i].tolist()
            if row != b or hop != l:
                raise ValueError(ROW_HOP)
            if not (0 <= head < n_ent and 0 <= tail < n_ent):
                raise ValueError(ENTITY)
            if not 0 <= rel < n_rela_rows:
                raise ValueError(RELATION)
            if last is not None and tail < last:
                raise ValueError(ORDER)
            last = tail
            if (keep is None or keep[i]) and (b * n_ent + head) in where:
                at.append(i)
                src.append(where[b * n_ent + head])
    at = np.array(at, np.int64)
    keys, dst_ptr = [], []
    for j, i in enumerate(at.tolist()):
        k = int(e[i, 0]) * n_ent + int(e[i, 4])
        if not keys or keys[-1] != k:
            if l == L and keys and keys[-1] // n_ent == k // n_ent:
                raise ValueError(TWO_TAILS)
            keys.append(k)
            dst_ptr.append(j)
    keys = np.array(keys, np.int64)
    return dict(at=at.astype(np.int32), src=np.array(src, np.int32), rel=e[at, 3].astype(np.int32),
                time=None if edge_time is None else np.asarray(edge_time)[at].astype(np.int32), keys=keys,
                dst_ptr=np.array(dst_ptr + [len(at)], np.int32) if len(at) else np.zeros(0, np.int32), row_of=(keys // n_ent).astype(np.int32),
                prev_idx=np.array([where.get(int(k), -1) for k in keys.tolist()], np.int32))
