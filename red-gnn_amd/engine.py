"""Thin host objects over the C-ABI handles: ``Graph`` (rg_graph) and ``Frontier`` (rg_frontier).

PyTorch is used here for device memory and the current HIP stream only; every computation
below is a call into libredgnn.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


# tests set this to 1 (per-query walk) or 2..5 (word-parallel, 32/16/8/4 queries per item) to force rg_layer_fwd's edge walk; 0 = the
# library picks from the hop's sizes (8, the single-source walk, on hop 0 of a batch of queries)
FORCE_WALK = 0

# bench.py sets these to lists to collect (start_event, end_event, n_edges, n_new) per rg_layer_fwd launch and
# (start_event, end_event, n_rows) per rg_dense_fwd launch
KERNEL_EVENTS = None
DENSE_EVENTS = None
# ... and (start_event, end_event, n_edges, n_old) per rg_layer_bwd call (its kernels: layer_bwd_kernel, bwd_combine_kernel, key_bwd_kernel)
BWD_EVENTS = None
# tools/probe_explain.py sets this to a list to collect (start_event, end_event, level, n_edges) per hop of explain_hop
EXPLAIN_EVENTS = None
# tools/probe_profile.py sets this to a list to collect (start_event, end_event, level) per attn_profile call
PROFILE_EVENTS = None


def _require_gpu(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.NativeError("red_gnn_amd runs on an MI355X (device 'cuda'); got device %r. "
                               "There is no CPU path in the product — the CPU restatement lives in oracle/ for tests only."
                               % (device,))
    if not torch.cuda.is_available():
        raise _lib.NativeError("red_gnn_amd needs an MI355X: no ROCm device is visible to this process. The HIP path has "
                               "no CPU fallback (the CPU restatement in oracle/ is test infrastructure only).")
    return device


_GRAPH_SERIAL = [0]


def _next_serial():
    _GRAPH_SERIAL[0] += 1
    return _GRAPH_SERIAL[0]


class Graph:
    """Device-resident KG (inverse + identity rows added, CSR by head and by tail).
    Replaces load_data.py:69-81 (double_triple + load_graph).  ``serial`` is unique per object for the life of the process (caches key
    on it: id() of a collected graph can come back)."""

    def __init__(self, n_ent, n_rel, triples, add_inverse=True, device="cuda"):
        self.serial = _next_serial()
        self.device = _require_gpu(device)
        trip = np.ascontiguousarray(np.asarray(triples, dtype=np.int32).reshape(-1, 3))
        self.n_ent, self.n_rel = int(n_ent), int(n_rel)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rg_graph_create(self.n_ent, self.n_rel, _lib.ptr(trip), len(trip),
                                                  1 if add_inverse else 0, C.byref(h)))
        self.handle = h
        self.n_fact = int(_lib.lib().rg_graph_n_fact(h))

    @classmethod
    def from_device(cls, n_ent, n_rel, triples_dev, add_inverse=True):
        """The same graph built on the device from a device int32 [n,3] tensor (rg_graph_create_device): the per-epoch rebuild of
        shuffle_train without a host round trip of the triples."""
        self = cls.__new__(cls)
        self.serial = _next_serial()
        self.device = _require_gpu(triples_dev.device)
        assert triples_dev.dtype == torch.int32 and triples_dev.dim() == 2 and triples_dev.shape[1] == 3
        trip = triples_dev.contiguous()
        self.n_ent, self.n_rel = int(n_ent), int(n_rel)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rg_graph_create_device(self.n_ent, self.n_rel, _lib.ptr(trip), trip.shape[0], 1 if add_inverse else 0,
                                                         _lib.stream_ptr(), C.byref(h)))
        self.handle = h
        self.n_fact = int(_lib.lib().rg_graph_n_fact(h))
        return self

    def export_packs(self):
        """(vrows [n_vrows,4], ent [n_packs*128,2], pack [n_packs,4], rows [n_vrows,2]) of the word-parallel walk as numpy — for tests."""
        L = _lib.lib()
        n_packs, n_vrows = C.c_int32(), C.c_int32()
        _lib.check(L.rg_graph_export_packs(self.handle, C.byref(n_packs), C.byref(n_vrows), None, None, None, None))
        vr = np.empty((n_vrows.value, 4), np.int32)
        ent = np.empty((n_packs.value * 128, 2), np.int32)
        pack = np.empty((n_packs.value, 4), np.int32)
        rows = np.empty((n_vrows.value if n_packs.value else 0, 2), np.int32)      # (a graph without packs has no pack rows: nothing is copied)
        _lib.check(L.rg_graph_export_packs(self.handle, None, None, _lib.ptr(ent), _lib.ptr(pack), _lib.ptr(rows), _lib.ptr(vr)))
        return vr, ent, pack, rows

    def export(self):
        """(out_ptr, out_rel_tail[n_fact,2], in_ptr, in_head_rel[n_fact,2]) as numpy — for tests."""
        op = np.empty(self.n_ent + 1, np.int32)
        ip = np.empty(self.n_ent + 1, np.int32)
        ort = np.empty((self.n_fact, 2), np.int32)
        ihr = np.empty((self.n_fact, 2), np.int32)
        _lib.check(_lib.lib().rg_graph_export(self.handle, _lib.ptr(op), _lib.ptr(ort), _lib.ptr(ip), _lib.ptr(ihr)))
        return op, ort, ip, ihr

    def export_out_by_tail(self):
        """(rel_tail [n_fact,2], pos [n_fact]) of the out-list ordered by (tail, CSR-by-tail position) as numpy — for tests.  Rows by
        export()'s out_ptr; pos indexes export()'s in_head_rel."""
        rt = np.empty((self.n_fact, 2), np.int32)
        pos = np.empty(self.n_fact, np.int32)
        _lib.check(_lib.lib().rg_graph_export_out_by_tail(self.handle, _lib.ptr(rt), _lib.ptr(pos), None))
        return rt, pos

    EXPORT_SCALARS = ("n_fact", "max_in_deg", "max_out_deg") + tuple("%s_vr_%s" % (d, f) for d in ("in", "out", "rel", "time")
                                                                    for f in ("n", "n_split", "n_slots"))
    EXPORT_ARRAYS = ("rel_ptr", "rel_ht", "rel_tm", "time_ptr", "time_ht", "time_rel", "in_pk", "out_pk", "out_bt_pk") + \
        tuple("%s_vr_%s" % (d, f) for d in ("in", "out", "rel", "time") for f in ("rows", "split"))

    def export_all(self):
        """Every array and scalar of the graph as a dict of numpy arrays and ints — for tests.  What export (out_ptr, out_rel_tail,
        in_ptr, in_head_rel), export_out_by_tail (out_bt_rel_tail, out_bt_pos), export_time (out_time, in_time) and export_packs
        (pack_ent, pack, pack_rows; its vrows are in_vr_rows) give, the EXPORT_ARRAYS of rg_graph_export_array and its EXPORT_SCALARS.
        An array the graph does not have (the out-list by tail of a temporal graph, the time arrays of a static one, packed entries
        of a wide one) is None; a graph without packs has pack arrays of length 0."""
        L = _lib.lib()
        d = dict(zip(("out_ptr", "out_rel_tail", "in_ptr", "in_head_rel"), self.export()))
        temporal = bool(getattr(self, "n_time", 0))
        d["out_bt_rel_tail"], d["out_bt_pos"] = (None, None) if temporal else self.export_out_by_tail()
        d["out_time"], d["in_time"] = self.export_time() if temporal else (None, None)
        _, d["pack_ent"], d["pack"], d["pack_rows"] = self.export_packs()
        scalars = np.zeros(len(self.EXPORT_SCALARS), np.int64)
        _lib.check(L.rg_graph_export_array(self.handle, None, None, None, _lib.ptr(scalars)))
        d.update((k, int(v)) for k, v in zip(self.EXPORT_SCALARS, scalars))
        for name in self.EXPORT_ARRAYS:
            dims = np.zeros(2, np.int64)
            _lib.check(L.rg_graph_export_array(self.handle, name.encode(), _lib.ptr(dims), None, None))
            if dims[0] < 0:
                d[name] = None
                continue
            a = np.empty((int(dims[0]), int(dims[1])), np.uint32 if name.endswith("_pk") else np.int32)
            _lib.check(L.rg_graph_export_array(self.handle, name.encode(), None, _lib.ptr(a), None))
            d[name] = a.reshape(-1) if dims[1] == 1 else a
        return d

    def close(self):
        if getattr(self, "handle", None) is not None and _lib._lib is not None:
            _lib.lib().rg_graph_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TemporalGraph(Graph):
    """Device-resident quadruple graph (head, rel, tail, time id) of T-RED-GNN (Temporal/interpolation/graph.py:34-49),
    used as given: the reference's array already holds the identity rows with the sentinel timestamp."""

    def __init__(self, n_ent, n_rela_rows, n_time, quads, device="cuda", exclude=None):
        """``exclude``: row indices of ``quads`` to leave out (the training mode's np.delete, done while the rows are read)."""
        self.serial = _next_serial()
        self.device = _require_gpu(device)
        q = quads if (isinstance(quads, np.ndarray) and quads.dtype == np.int32 and quads.flags.c_contiguous and quads.ndim == 2) \
            else np.ascontiguousarray(np.asarray(quads, dtype=np.int32).reshape(-1, 4))
        self.n_ent, self.n_rel, self.n_rela_rows, self.n_time = int(n_ent), 0, int(n_rela_rows), int(n_time)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if exclude is None:
                _lib.check(_lib.lib().rg_tgraph_create(self.n_ent, self.n_rela_rows, self.n_time, _lib.ptr(q), len(q), C.byref(h)))
            else:
                ex = np.ascontiguousarray(np.asarray(exclude, dtype=np.int64).reshape(-1))
                _lib.check(_lib.lib().rg_tgraph_create_excluding(self.n_ent, self.n_rela_rows, self.n_time, _lib.ptr(q), len(q),
                                                                 _lib.ptr(ex), len(ex), C.byref(h)))
        self.handle = h
        self.n_fact = int(_lib.lib().rg_graph_n_fact(h))
        self._rows = (q, None if exclude is None else ex)      # a reference to the caller's rows: default_anchors reads them once
        self._anchors = None

    def default_anchors(self):
        """int64 [S, 2] = (entity, time id) sorted by (time, entity): the distinct (head, time) pairs of the graph's rows whose
        relation is not the identity (n_rela_rows - 1), the anchors trule_ground counts over when given none.  Formed on first use
        from the rows given at construction (kept by reference), then cached."""
        if self._anchors is None:
            q, ex = self._rows
            if ex is not None:
                q = np.delete(q, ex, axis=0)
            q = q[q[:, 1] != self.n_rela_rows - 1]
            key = np.unique(q[:, 3].astype(np.int64) * self.n_ent + q[:, 0])
            self._anchors = np.stack([key % self.n_ent, key // self.n_ent], 1)
            self._rows = None
        return self._anchors

    def export_time(self):
        """(out_time [n_fact], in_time [n_fact]): the time id of every entry of export()'s out_rel_tail / in_head_rel — for tests."""
        ot = np.empty(self.n_fact, np.int32)
        it = np.empty(self.n_fact, np.int32)
        _lib.check(_lib.lib().rg_graph_export_time(self.handle, _lib.ptr(ot), _lib.ptr(it)))
        return ot, it


class Frontier:
    """Per-batch visited-set state (levels of (batch, entity) node sets) in a torch-owned workspace.
    Replaces the state threaded through RED_GNN_trans.forward / DataLoader.get_neighbors
    (models.py:73-78, load_data.py:106-131)."""

    def __init__(self, n_ent, batch, n_levels=2, device="cuda"):
        self.device = _require_gpu(device)
        L = _lib.lib()
        self.n_ent, self.batch, self.n_levels = int(n_ent), int(batch), int(n_levels)
        nbytes = L.rg_frontier_workspace_bytes(self.n_ent, self.batch, self.n_levels)
        if nbytes == 0:
            raise _lib.NativeError("bad frontier shape n_ent=%d batch=%d n_levels=%d" % (n_ent, batch, n_levels))
        self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = self.workspace.data_ptr()
        aligned = (base + 255) // 256 * 256
        h = C.c_void_p()
        _lib.check(L.rg_frontier_create(self.n_ent, self.batch, self.n_levels, C.c_void_p(aligned), nbytes, C.byref(h)))
        self.handle = h
        self._counts = (C.c_int64 * 4)()
        self.level = -1
        self.n_new = self.n_old = self.n_edges = 0
        self.generation = 0      # bumped by every reset: the level bitmaps of an older generation are gone
        self.leases = 0          # live FrontierLease objects (autograd graphs whose backward still reads the level bitmaps)

    def reset(self, q_sub):
        """Level 0 = {(b, q_sub[b])} (models.py:73).  q_sub: int32 device tensor [batch]."""
        assert q_sub.dtype == torch.int32 and q_sub.is_cuda and q_sub.numel() == self.batch
        _lib.check(_lib.lib().rg_frontier_reset(self.handle, _lib.ptr(q_sub), _lib.stream_ptr()))
        self.level, self.n_new, self.n_old, self.n_edges = 0, self.batch, 0, 0
        self.generation += 1

    def reset_nodes(self, nodes):
        """Level 0 = an arbitrary node set, int32 device tensor [n,2] (batch, entity)."""
        assert nodes.dtype == torch.int32 and nodes.is_cuda and nodes.dim() == 2 and nodes.shape[1] == 2
        nodes = nodes.contiguous()
        _lib.check(_lib.lib().rg_frontier_reset_nodes(self.handle, _lib.ptr(nodes), nodes.shape[0], _lib.stream_ptr()))
        self.level, self.n_new, self.n_old, self.n_edges = 0, nodes.shape[0], 0, 0
        self.generation += 1

    def set_window(self, win_lo, win_hi, n_data):
        """Per-query data-row windows of the extrapolation setting (rg_frontier_set_window); int32 device tensors [batch], kept alive here."""
        if win_lo is None:
            self._window = None
            _lib.check(_lib.lib().rg_frontier_set_window(self.handle, None, None, 0))
            return
        assert win_lo.dtype == torch.int32 and win_hi.dtype == torch.int32 and win_lo.is_cuda and win_lo.numel() == self.batch == win_hi.numel()
        self._window = (win_lo.contiguous(), win_hi.contiguous())
        _lib.check(_lib.lib().rg_frontier_set_window(self.handle, _lib.ptr(self._window[0]), _lib.ptr(self._window[1]), int(n_data)))

    def expand(self, graph):
        """One hop.  Returns (n_new, n_edges, n_old); synchronises the stream once."""
        _lib.check(_lib.lib().rg_frontier_expand(self.handle, graph.handle, self._counts, _lib.stream_ptr()))
        self.n_new, self.n_edges, self.n_old, self.level = (int(self._counts[i]) for i in range(4))
        return self.n_new, self.n_edges, self.n_old

    def expand_async(self, graph):
        """One hop with no read-back (rg_frontier_expand_async): nothing synchronises; the sizes stay on the device
        (count_ptr, level_counts) and self.n_new / n_old / n_edges are unknown (-1) until level_counts() is called."""
        _lib.check(_lib.lib().rg_frontier_expand_async(self.handle, graph.handle, _lib.stream_ptr()))
        self.level += 1
        self.n_new = self.n_old = self.n_edges = -1

    def expand_nodes_async(self, graph, nodes, prev, edge_hint=None):
        """expand_async + nodes_into in one library call (rg_frontier_expand_nodes_async: one fused launch for small batches)."""
        _lib.check(_lib.lib().rg_frontier_expand_nodes_async(self.handle, graph.handle, _lib.ptr(nodes), _lib.ptr(prev), _lib.stream_ptr()))
        if edge_hint is not None and edge_hint >= 0:      # what an eager run of the same shape counted: tunes the next layer call's tickets
            _lib.check(_lib.lib().rg_frontier_set_edge_hint(self.handle, int(edge_hint)))
        self.level += 1
        self.n_new = self.n_old = self.n_edges = -1

    def count_ptr(self):
        """Device address of the newest level's node count (int32), for dense_fwd_dev."""
        return C.c_void_p(_lib.lib().rg_frontier_count_ptr(self.handle))

    def level_counts(self):
        """[(N_l, E_l) for l = 0..level] read back from the device (synchronises the stream)."""
        buf = (C.c_int64 * 32)()
        _lib.check(_lib.lib().rg_frontier_level_counts(self.handle, buf, _lib.stream_ptr()))
        return [(int(buf[2 * l]), int(buf[2 * l + 1])) for l in range(self.level + 1)]

    def nodes_into(self, nodes, prev):
        """rg_frontier_nodes into caller-owned buffers of capacity batch * n_ent rows (no size needed on the host)."""
        _lib.check(_lib.lib().rg_frontier_nodes(self.handle, _lib.ptr(nodes), _lib.ptr(prev), None, _lib.stream_ptr()))

    def nodes(self, want_prev=True, want_old_new=True):
        """(nodes int32 [n_new,2] sorted, prev_idx int32 [n_new] or None, old_nodes_new_idx int32 [n_old] or None)."""
        nodes = torch.empty((self.n_new, 2), dtype=torch.int32, device=self.device)
        prev = torch.empty(self.n_new, dtype=torch.int32, device=self.device) if want_prev else None
        old_new = (torch.empty(self.n_old, dtype=torch.int32, device=self.device)
                   if (want_old_new and self.level > 0) else None)
        _lib.check(_lib.lib().rg_frontier_nodes(self.handle, _lib.ptr(nodes), _lib.ptr(prev), _lib.ptr(old_new),
                                                _lib.stream_ptr()))
        return nodes, prev, old_new

    def edges(self, graph, nodes_new, level=None):
        """Materialised (batch, head, rel, tail, old_idx, new_idx) int32 [E,6] + row_ptr [n_new+1]
        of hop level-1 -> level (destination-segmented)."""
        level = self.level if level is None else level
        n_new = nodes_new.shape[0]
        L = _lib.lib()
        scratch = torch.empty(L.rg_frontier_edges_scratch_bytes(n_new), dtype=torch.uint8, device=self.device)
        row_ptr = torch.empty(n_new + 1, dtype=torch.int32, device=self.device)
        # pass 1: counts only -> E
        _lib.check(L.rg_frontier_edges(self.handle, graph.handle, level, _lib.ptr(nodes_new), n_new, None,
                                       _lib.ptr(row_ptr), _lib.ptr(scratch), _lib.stream_ptr()))
        n_e = int(row_ptr[-1].item())
        edges = torch.empty((n_e, 6), dtype=torch.int32, device=self.device)
        _lib.check(L.rg_frontier_edges(self.handle, graph.handle, level, _lib.ptr(nodes_new), n_new, _lib.ptr(edges),
                                       _lib.ptr(row_ptr), _lib.ptr(scratch), _lib.stream_ptr()))
        return edges, row_ptr

    def scratch(self, nbytes):
        """A reusable device scratch buffer of at least nbytes (kernels' partial-sum space)."""
        buf = getattr(self, "_scratch", None)
        if buf is None or buf.numel() < nbytes:
            buf = self._scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return buf

    def close(self):
        if getattr(self, "handle", None) is not None and _lib._lib is not None:
            _lib.lib().rg_frontier_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrontierLease:
    """Held by the autograd contexts of one grad-enabled forward: while it lives, the frontier's level bitmaps are still
    needed by that graph's backward (rg_layer_bwd / rg_tlayer_bwd revisit every hop), so the per-shape caches hand out another
    Frontier instead of resetting this one (two forwards before the first backward: gradient accumulation, two losses).
    ``check()`` in backward turns any remaining misuse (a reset behind the lease's back) into a clear error."""
    __slots__ = ("frontier", "generation", "released")

    def __init__(self, frontier):
        self.frontier, self.generation, self.released = frontier, frontier.generation, False
        frontier.leases += 1

    def release(self):
        """Called when the first hop's backward has run (the last one of a backward pass): autograd frees saved tensors then, but
        keeps the contexts - and this object - for as long as the forward's output tensor lives.  A second backward through a
        retained graph is still guarded by check()."""
        if not self.released:
            self.released = True
            self.frontier.leases -= 1

    def check(self):
        if self.frontier.generation != self.generation:
            raise RuntimeError("red_gnn_amd: the frontier of this autograd graph was reset by a later forward (generation %d, now %d); "
                               "its level bitmaps are gone, the backward cannot run" % (self.generation, self.frontier.generation))

    def __del__(self):
        self.release()


class FrontierPool:
    """Frontiers per shape key; ``get`` returns one that no live autograd graph leases (allocating another if needed)."""

    def __init__(self, max_keys=64):      # (8 evaluation lanes x a few batch shapes)
        self.max_keys, self.pool = max_keys, {}

    def get(self, n_ent, batch, n_levels, device):
        # per stream: forwards enqueued on different streams (the evaluator's lanes) run concurrently on the device
        key = (n_ent, batch, n_levels, str(device), torch.cuda.current_stream(device).cuda_stream)
        frs = self.pool.get(key)
        if frs is None:
            if len(self.pool) >= self.max_keys:
                self.pool = {k: [f for f in v if f.leases > 0] for k, v in self.pool.items()}
                self.pool = {k: v for k, v in self.pool.items() if v}
            frs = self.pool[key] = []
        for fr in frs:
            if fr.leases == 0:
                return fr
        fr = Frontier(n_ent, batch, n_levels, device)
        frs.append(fr)
        return fr

    def clear(self):
        self.pool = {}


def layer_fwd(frontier, graph, level, nodes_new, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim):
    """agg [n_new, ld] = fused message passing of hop level-1 -> level (rg_layer_fwd)."""
    ld, ap = hidden.shape[1], a_s.shape[1]
    for t in (hidden, rela, a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert rela.shape[1] == ld and a_r.shape[1] == ap and a_q.shape[1] == ap
    n_new = nodes_new.shape[0]
    agg = torch.empty((n_new, ld), dtype=torch.float32, device=hidden.device)
    nbytes = _lib.lib().rg_layer_fwd_scratch_bytes(frontier.handle, graph.handle, ld)
    scratch = frontier.scratch(nbytes)
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_layer_fwd(frontier.handle, graph.handle, level, n_new,
                                       _lib.ptr(hidden), _lib.ptr(rela), d, ld, _lib.ptr(a_s), _lib.ptr(a_r),
                                       _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim,
                                       _lib.ptr(agg), _lib.ptr(scratch), nbytes, FORCE_WALK, _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append((ev[0], ev[1], frontier.n_edges, n_new))
    return agg


def explain_seed(frontier, level, objs):
    """rg_explain_seed: (marks int32 [B, W] words = {(b, objs[b])} where objs[b] is in level `level`, reached bool [B])."""
    assert objs.dtype == torch.int32 and objs.is_cuda and objs.numel() == frontier.batch
    W = (frontier.n_ent + 31) // 32
    marks = torch.empty((frontier.batch, W), dtype=torch.int32, device=frontier.device)
    reached = torch.empty(frontier.batch, dtype=torch.bool, device=frontier.device)
    _lib.check(_lib.lib().rg_explain_seed(frontier.handle, frontier.batch, frontier.n_ent, level, _lib.ptr(objs.contiguous()),
                                          _lib.ptr(marks), _lib.ptr(reached), _lib.stream_ptr()))
    return marks, reached


def explain_hop(frontier, graph, level, marks, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, min_alpha):
    """One hop of the r-digraph extraction (rg_explain_count + rg_explain_emit): the hop-`level` edges into the marked tails whose head
    is in level-1 and whose attention is >= min_alpha.  Returns (marks of their heads [B, W], edges int32 [E, 4] = (row, head, rel, tail)
    in (row, tail, CSR position) order, alpha [E])."""
    for t in (a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    ap = a_s.shape[1]
    assert a_r.shape[1] == ap and a_q.shape[1] == ap
    L, dev = _lib.lib(), frontier.device
    marks_prev = torch.empty_like(marks)
    word_ptr = torch.empty(marks.numel() + 1, dtype=torch.int32, device=dev)
    scratch = frontier.scratch(L.rg_explain_scratch_bytes(frontier.handle) + 256)
    base = scratch.data_ptr()
    aligned = (base + 255) // 256 * 256
    n_e = C.c_int64()
    args = (frontier.handle, graph.handle, frontier.batch, frontier.n_ent, level, _lib.ptr(marks), _lib.ptr(a_s), _lib.ptr(a_r),
            _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim, float(min_alpha))
    ev = None
    if EXPLAIN_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(L.rg_explain_count(*args, _lib.ptr(marks_prev), _lib.ptr(word_ptr), C.c_void_p(aligned),
                                  scratch.numel() - (aligned - base), C.byref(n_e), _lib.stream_ptr()))
    edges = torch.empty((n_e.value, 4), dtype=torch.int32, device=dev)
    alpha = torch.empty(n_e.value, dtype=torch.float32, device=dev)
    if n_e.value:
        _lib.check(L.rg_explain_emit(*args, _lib.ptr(word_ptr), _lib.ptr(edges), _lib.ptr(alpha), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        EXPLAIN_EVENTS.append((ev[0], ev[1], level, n_e.value))
    return marks_prev, edges, alpha


def texplain_hop(frontier, graph, level, marks, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, min_alpha, entry="rg_texplain"):
    """explain_hop on a temporal graph (rg_texplain_count + rg_texplain_emit).  Returns (marks of the heads [B, W], edges int32 [E, 4] =
    (row, head, rel, tail) in (row, tail, CSR position) order, alpha [E], time int32 [E] = the edges' time ids)."""
    count, emit = getattr(_lib.lib(), entry + "_count"), getattr(_lib.lib(), entry + "_emit")
    for t in (a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    ap = a_s.shape[1]
    assert a_r.shape == (graph.n_rela_rows, ap) and a_q.shape == (frontier.batch, ap)
    L, dev = _lib.lib(), frontier.device
    marks_prev = torch.empty_like(marks)
    word_ptr = torch.empty(marks.numel() + 1, dtype=torch.int32, device=dev)
    scratch = frontier.scratch(L.rg_explain_scratch_bytes(frontier.handle) + 256)
    base = scratch.data_ptr()
    aligned = (base + 255) // 256 * 256
    n_e = C.c_int64()
    args = (frontier.handle, graph.handle, frontier.batch, frontier.n_ent, level, _lib.ptr(marks), _lib.ptr(a_s), _lib.ptr(a_r),
            _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim, float(min_alpha))
    ev = None
    if EXPLAIN_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(count(*args, _lib.ptr(marks_prev), _lib.ptr(word_ptr), C.c_void_p(aligned),
                                   scratch.numel() - (aligned - base), C.byref(n_e), _lib.stream_ptr()))
    edges = torch.empty((n_e.value, 4), dtype=torch.int32, device=dev)
    alpha = torch.empty(n_e.value, dtype=torch.float32, device=dev)
    time = torch.empty(n_e.value, dtype=torch.int32, device=dev)
    if n_e.value:
        _lib.check(emit(*args, _lib.ptr(word_ptr), _lib.ptr(edges), _lib.ptr(alpha), _lib.ptr(time), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        EXPLAIN_EVENTS.append((ev[0], ev[1], level, n_e.value))
    return marks_prev, edges, alpha, time


def xexplain_hop(frontier, graph, level, marks, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, min_alpha):
    """explain_hop of the extrapolation model (rg_xexplain_count + rg_xexplain_emit) on a frontier with its row windows set: as
    texplain_hop, the fourth result being the edges' data rows int32 [E] (>= the number of data rows for a self-loop)."""
    return texplain_hop(frontier, graph, level, marks, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, min_alpha, entry="rg_xexplain")


def explain_gather(hop, batch, edges, alpha, row_first, row_base, edges_out, alpha_out):
    """rg_explain_gather: one hop's (row, head, rel, tail) list into the (row, hop, head, rel, tail) layout of edges_out [n_out, 5]:
    edge i of row b goes to row_base[b] + i - row_first[b] (int64 [batch] each)."""
    assert edges.dtype == torch.int32 and edges.is_contiguous() and edges_out.is_contiguous() and alpha_out.is_contiguous()
    assert row_first.dtype == torch.int64 and row_base.dtype == torch.int64
    _lib.check(_lib.lib().rg_explain_gather(edges.shape[0], hop, batch, _lib.ptr(edges), _lib.ptr(alpha.contiguous()),
                                            _lib.ptr(row_first.contiguous()), _lib.ptr(row_base.contiguous()), edges_out.shape[0],
                                            _lib.ptr(edges_out), _lib.ptr(alpha_out), _lib.stream_ptr()))


def attn_profile(frontier, graph, level, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, sum_out, count_out):
    """rg_attn_profile: adds the hop-`level` edges of every query into sum_out / count_out (int64 [B, n_rela_rows], zeroed by the
    caller): per edge relation the number of edges and the sum of llrintf(alpha * 2^32).  Integer sums: bit-identical whatever the
    schedule, the split of the batch or the order of its queries."""
    for t in (a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    ap = a_s.shape[1]
    assert a_r.shape == (2 * graph.n_rel + 1, ap) and a_q.shape == (frontier.batch, ap)      # (the kernel's bins: the graph's rows)
    for t in (sum_out, count_out):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.shape == (frontier.batch, a_r.shape[0])
    ev = None
    if PROFILE_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_attn_profile(frontier.handle, graph.handle, frontier.batch, frontier.n_ent, level, a_s.shape[0],
                                          _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha),
                                          attn_dim, _lib.ptr(sum_out), _lib.ptr(count_out), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        PROFILE_EVENTS.append((ev[0], ev[1], level))


def tattn_profile(frontier, graph, level, q_time, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, sum_out, count_out):
    """rg_tattn_profile: attn_profile on a temporal graph with the edge direction as an axis.  Adds the hop-`level` edges of every query
    into sum_out / count_out (int64 [B, 3, n_rela_rows], zeroed by the caller): direction 0 past / 1 now / 2 future of the edge's time
    against q_time[b] (int32 [B])."""
    for t in (a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    ap = a_s.shape[1]
    assert a_r.shape == (graph.n_rela_rows, ap) and a_q.shape == (frontier.batch, ap)      # (the kernel's bins: the graph's rows)
    assert q_time.is_cuda and q_time.dtype == torch.int32 and q_time.is_contiguous() and q_time.numel() == frontier.batch
    for t in (sum_out, count_out):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.shape == (frontier.batch, 3, a_r.shape[0])
    ev = None
    if PROFILE_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_tattn_profile(frontier.handle, graph.handle, frontier.batch, frontier.n_ent, level, a_s.shape[0],
                                           _lib.ptr(q_time), _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q), ap, _lib.ptr(w_alpha),
                                           _lib.ptr(b_alpha), attn_dim, _lib.ptr(sum_out), _lib.ptr(count_out), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        PROFILE_EVENTS.append((ev[0], ev[1], level))


def xattn_profile(frontier, graph, level, q_time, loop_time, row_time, lag_bin, n_bins, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, sum_out,
                  count_out):
    """rg_xattn_profile: attn_profile of the extrapolation model on a frontier with its row windows set, with the edge's binned lag as an
    axis.  Adds the hop-`level` edges of every query into sum_out / count_out (int64 [B, n_bins, n_rela_rows], zeroed by the caller):
    bin = lag_bin[the forward's time-table row of the edge] (lag_bin uint8 [n_lag]; an entry >= n_bins drops the edge), the row being
    q_time[b] - row_time[data row], or q_time[b] - loop_time[b] for a self-loop, clamped to 0..n_lag - 1 (int32 tensors)."""
    for t in (a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    ap = a_s.shape[1]
    assert a_r.shape == (graph.n_rela_rows, ap) and a_q.shape == (frontier.batch, ap)      # (the kernel's bins: the graph's rows)
    for t in (q_time, loop_time, row_time):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    assert q_time.numel() == frontier.batch and loop_time.numel() == frontier.batch
    assert lag_bin.is_cuda and lag_bin.dtype == torch.uint8 and lag_bin.is_contiguous() and lag_bin.dim() == 1 and lag_bin.numel() >= 1
    for t in (sum_out, count_out):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.shape == (frontier.batch, n_bins, a_r.shape[0])
    ev = None
    if PROFILE_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_xattn_profile(frontier.handle, graph.handle, frontier.batch, frontier.n_ent, level, a_s.shape[0],
                                           _lib.ptr(q_time), _lib.ptr(loop_time), _lib.ptr(row_time), _lib.ptr(lag_bin), lag_bin.numel(),
                                           int(n_bins), _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q), ap, _lib.ptr(w_alpha),
                                           _lib.ptr(b_alpha), attn_dim, _lib.ptr(sum_out), _lib.ptr(count_out), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        PROFILE_EVENTS.append((ev[0], ev[1], level))


def layer_fwd_plan(frontier, graph, level, n_old, n_new, n_edges, ld):
    """The general walk (1 .. 7) rg_layer_fwd picks for a hop of these sizes (rg_layer_fwd_plan)."""
    return int(_lib.lib().rg_layer_fwd_plan(frontier.handle, graph.handle, level, n_old, n_new, n_edges, ld))


def layer_fwd_walk(frontier, graph, level, n_old, n_new, n_edges, ld):
    """The walk rg_layer_fwd's walk 0 runs on this hop: 8 (single-source walk) where it applies, else the general plan.  Recorded from
    an eager forward for graph replay."""
    if _lib.lib().rg_layer_fwd_single_source(frontier.handle, graph.handle, level):
        return 8
    return layer_fwd_plan(frontier, graph, level, n_old, n_new, n_edges, ld)


def layer_fwd_scratch_bytes(frontier, graph, ld):
    return _lib.lib().rg_layer_fwd_scratch_bytes(frontier.handle, graph.handle, ld)


def layer_fwd_into(frontier, graph, level, n_hint, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, agg, scratch, walk=1):
    """rg_layer_fwd after expand_async: agg has room for batch * n_ent rows; the sizes are not known on the host, so the caller
    names the walk (recorded from an eager forward of the same shape) and n_hint (> 0) picks the per-query walk's flavour."""
    ld, ap = hidden.shape[1], a_s.shape[1]
    _lib.check(_lib.lib().rg_layer_fwd(frontier.handle, graph.handle, level, max(int(n_hint), 1),
                                       _lib.ptr(hidden), _lib.ptr(rela), d, ld, _lib.ptr(a_s), _lib.ptr(a_r),
                                       _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim,
                                       _lib.ptr(agg), _lib.ptr(scratch), scratch.numel(), FORCE_WALK or max(int(walk), 1), _lib.stream_ptr()))


def tlayer_fwd(frontier, graph, level, n_new, q_time, hidden_dir, rela_dir, time_dir, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim):
    """Temporal fused message passing (rg_tlayer_fwd): agg [n_new, ld]."""
    ld, ap = hidden_dir.shape[1], a_s.shape[1]
    for t in (hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert q_time.dtype == torch.int32 and q_time.is_cuda
    agg = torch.empty((n_new, ld), dtype=torch.float32, device=hidden_dir.device)
    nbytes = _lib.lib().rg_layer_fwd_scratch_bytes(frontier.handle, graph.handle, ld)
    scratch = frontier.scratch(nbytes)
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_tlayer_fwd(frontier.handle, graph.handle, level, n_new, _lib.ptr(q_time), _lib.ptr(hidden_dir),
                                        _lib.ptr(rela_dir), _lib.ptr(time_dir), d, ld, _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q),
                                        ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim, _lib.ptr(agg), _lib.ptr(scratch),
                                        nbytes, _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append((ev[0], ev[1], frontier.n_edges, n_new))
    return agg


def xlayer_fwd(frontier, graph, level, n_new, q_time, loop_time, row_time, n_data, hidden_p, rela_p, time_p, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim):
    """Temporal-extrapolation fused message passing (rg_xlayer_fwd): agg [n_new, ld]."""
    ld, ap = hidden_p.shape[1], a_s.shape[1]
    for t in (hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha, b_alpha):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    for t in (q_time, loop_time, row_time):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    agg = torch.empty((n_new, ld), dtype=torch.float32, device=hidden_p.device)
    nbytes = _lib.lib().rg_layer_fwd_scratch_bytes(frontier.handle, graph.handle, ld)
    scratch = frontier.scratch(nbytes)
    ev = None
    if KERNEL_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_xlayer_fwd(frontier.handle, graph.handle, level, n_new, _lib.ptr(q_time), _lib.ptr(loop_time), _lib.ptr(row_time),
                                        int(n_data), _lib.ptr(hidden_p), _lib.ptr(rela_p), _lib.ptr(time_p), time_p.shape[0], d, ld,
                                        _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim,
                                        _lib.ptr(agg), _lib.ptr(scratch), nbytes, _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        KERNEL_EVENTS.append((ev[0], ev[1], frontier.n_edges, n_new))
    return agg


def layer_bwd(frontier, graph, level, nodes_old, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg):
    """Adjoint of layer_fwd (rg_layer_bwd).  Returns grads of (hidden, rela, a_s, a_r, a_q, w_alpha, b_alpha)."""
    ld, ap = hidden.shape[1], a_s.shape[1]
    grad_agg = grad_agg.contiguous()
    n_old = nodes_old.shape[0]
    dev = hidden.device
    g_h = torch.empty_like(hidden)
    g_as = torch.empty_like(a_s)
    g_rela = torch.zeros_like(rela)
    g_ar = torch.zeros_like(a_r)
    g_aq = torch.empty_like(a_q)
    g_w = torch.zeros(attn_dim, dtype=torch.float32, device=dev)
    g_b = torch.zeros(1, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().rg_layer_bwd_scratch_bytes(frontier.handle, graph.handle, ld, ap)
    scratch = frontier.scratch(nbytes)
    ev = None
    if BWD_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_layer_bwd(frontier.handle, graph.handle, level, n_old,
                                       _lib.ptr(hidden), _lib.ptr(rela), d, ld, _lib.ptr(a_s), _lib.ptr(a_r),
                                       _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim,
                                       _lib.ptr(grad_agg), _lib.ptr(g_h), _lib.ptr(g_rela), _lib.ptr(g_as),
                                       _lib.ptr(g_ar), _lib.ptr(g_aq), _lib.ptr(g_w), _lib.ptr(g_b), _lib.ptr(scratch), nbytes,
                                       _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        BWD_EVENTS.append((ev[0], ev[1], level, n_old))
    return g_h, g_rela, g_as, g_ar, g_aq, g_w, g_b


def tlayer_bwd(frontier, graph, level, n_old, q_time, hidden_dir, rela_dir, time_dir, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim,
               grad_agg):
    """Adjoint of tlayer_fwd (rg_tlayer_bwd).  Returns grads of (hidden_dir [3 n_old, ld], rela_dir, time_dir, a_s, a_r, a_q, w_alpha)."""
    ld, ap = hidden_dir.shape[1], a_s.shape[1]
    grad_agg = grad_agg.contiguous()
    dev = hidden_dir.device
    g_hd = torch.empty_like(hidden_dir)
    g_as = torch.empty_like(a_s)
    g_rd = torch.zeros_like(rela_dir)
    g_td = torch.zeros_like(time_dir)
    g_ar = torch.zeros_like(a_r)
    g_aq = torch.empty_like(a_q)
    g_w = torch.zeros(attn_dim, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().rg_tlayer_bwd_scratch_bytes(frontier.handle, graph.handle, ld, ap)
    scratch = frontier.scratch(nbytes)
    _lib.check(_lib.lib().rg_tlayer_bwd(frontier.handle, graph.handle, level, n_old, _lib.ptr(q_time), _lib.ptr(hidden_dir),
                                        _lib.ptr(rela_dir), _lib.ptr(time_dir), d, ld, _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q),
                                        ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim, _lib.ptr(grad_agg), _lib.ptr(g_hd),
                                        _lib.ptr(g_rd), _lib.ptr(g_td), _lib.ptr(g_as), _lib.ptr(g_ar), _lib.ptr(g_aq), _lib.ptr(g_w),
                                        _lib.ptr(scratch), nbytes, _lib.stream_ptr()))
    return g_hd, g_rd, g_td, g_as, g_ar, g_aq, g_w


def xlayer_bwd(frontier, graph, level, n_old, q_time, loop_time, row_time, n_data, hidden_p, rela_p, time_p, d, a_s, a_r, a_q, w_alpha,
               b_alpha, attn_dim, grad_agg):
    """Adjoint of xlayer_fwd (rg_xlayer_bwd).  Returns grads of (hidden_p [n_old, ld], rela_p, time_p, a_s, a_r, a_q, w_alpha)."""
    ld, ap = hidden_p.shape[1], a_s.shape[1]
    grad_agg = grad_agg.contiguous()
    dev = hidden_p.device
    g_hp = torch.empty_like(hidden_p)
    g_as = torch.empty_like(a_s)
    g_rp = torch.zeros_like(rela_p)
    g_tp = torch.zeros_like(time_p)
    g_ar = torch.zeros_like(a_r)
    g_aq = torch.empty_like(a_q)
    g_w = torch.zeros(attn_dim, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().rg_tlayer_bwd_scratch_bytes(frontier.handle, graph.handle, ld, ap)
    scratch = frontier.scratch(nbytes)
    _lib.check(_lib.lib().rg_xlayer_bwd(frontier.handle, graph.handle, level, n_old, _lib.ptr(q_time), _lib.ptr(loop_time), _lib.ptr(row_time),
                                        int(n_data), _lib.ptr(hidden_p), _lib.ptr(rela_p), _lib.ptr(time_p), time_p.shape[0], d, ld,
                                        _lib.ptr(a_s), _lib.ptr(a_r), _lib.ptr(a_q), ap, _lib.ptr(w_alpha), _lib.ptr(b_alpha), attn_dim,
                                        _lib.ptr(grad_agg), _lib.ptr(g_hp), _lib.ptr(g_rp), _lib.ptr(g_tp), _lib.ptr(g_as), _lib.ptr(g_ar),
                                        _lib.ptr(g_aq), _lib.ptr(g_w), _lib.ptr(scratch), nbytes, _lib.stream_ptr()))
    return g_hp, g_rp, g_tp, g_as, g_ar, g_aq, g_w


_GRAM_SCRATCH = {}


def gram_tn(g, x, colsum=False):
    """g^T x for node-row matrices g [N, m], x [N, n] (unit-stride columns; rows may be spaced: column blocks of wider buffers work
    without a copy), N in the millions: rg_gram_tn (exact fp32 MFMA products, rows read once, deterministic).  Returns out [m, n], or
    (out, column sums of g [m]) with colsum=True.  Products wider than 192 x 64 are tiled over column blocks."""
    assert g.is_cuda and x.is_cuda and g.dtype == torch.float32 and x.dtype == torch.float32 and g.shape[0] == x.shape[0]
    assert g.stride(1) == 1 and x.stride(1) == 1
    n_rows, m, n = g.shape[0], g.shape[1], x.shape[1]
    L = _lib.lib()
    out = torch.empty((m, n), dtype=torch.float32, device=g.device)
    cs = torch.empty(m, dtype=torch.float32, device=g.device) if colsum else None
    for m0 in range(0, m, 192):
        mc = min(192, m - m0)
        for n0 in range(0, n, 64):
            nc = min(64, n - n0)
            nbytes = L.rg_gram_tn_scratch_bytes(mc, nc)
            key = (str(g.device), torch.cuda.current_stream(g.device).cuda_stream)
            scratch = _GRAM_SCRATCH.get(key)
            if scratch is None or scratch.numel() < nbytes:
                scratch = _GRAM_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
            tile = out if (mc == m and nc == n) else torch.empty((mc, nc), dtype=torch.float32, device=g.device)
            cs_t = None
            if colsum and n0 == 0:
                cs_t = cs if mc == m else torch.empty(mc, dtype=torch.float32, device=g.device)
            gv, xv = g[:, m0:m0 + mc], x[:, n0:n0 + nc]
            _lib.check(L.rg_gram_tn(C.c_void_p(gv.data_ptr()), g.stride(0), mc, C.c_void_p(xv.data_ptr()), x.stride(0), nc, n_rows,
                                    _lib.ptr(tile), _lib.ptr(cs_t), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr()))
            if tile is not out:
                out[m0:m0 + mc, n0:n0 + nc] = tile
            if cs_t is not None and cs_t is not cs:
                cs[m0:m0 + mc] = cs_t
    return (out, cs) if colsum else out


_BLAS_CHOICE = [None]


def prefer_blas(n_rows):
    """Pick the GEMM library for the torch-side dense algebra of a training step from the number of node rows.
    hipBLASLt (torch's default on gfx950) searches its heuristics again for every new problem size: 75 us per call
    when the row count changes with every batch, as it does here, against 11 us through rocBLAS (tools/probe_small_gemm.py);
    with the family preset (20 queries per batch) that search was half of the step.  For millions of rows the batched
    weight-gradient products are 1.5x faster through hipBLASLt, and the call overhead no longer matters."""
    choice = "cublas" if n_rows < (1 << 17) else "cublaslt"      # torch's names: cublas = rocBLAS, cublaslt = hipBLASLt
    if _BLAS_CHOICE[0] != choice:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.backends.cuda.preferred_blas_library(choice)
        _BLAS_CHOICE[0] = choice


def dense_supported(d, attn_dim):
    return bool(_lib.lib().rg_dense_fwd_supported(d, attn_dim))


DENSE_PRECISIONS = {"f32": 0, "f16x2": 1, "f16x3": 2}


def dense_scratch(d, precision, device):
    """Scratch of rg_dense_fwd for this width and precision (d = 128 with split products: the weights' split image), or None."""
    nbytes = int(_lib.lib().rg_dense_scratch_bytes(d, DENSE_PRECISIONS[precision]))
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def dense_fwd(agg, hidden_prev, prev_idx, d, W_h, act, gate, Ws_next=None, attn_dim=0, ap=0, W_final=None, nodes=None,
              n_ent=0, scores_all=None, precision="f32", want_hidden=True):
    """Fused W_h + act + GRU step (+ next layer's a_s, + readout) on the matrix cores (rg_dense_fwd).  precision: "f32" = exact
    fp32 MFMA, "f16x3" = exact three-term f16 splits of every operand (fp32 arithmetic on the f16 pipe), "f16x2" = two-term f16
    splits (22 bits, fp32 accumulation); see include/redgnn.h.
    want_hidden=False (last layer only: W_final given, no Ws_next): the new state is neither allocated nor stored.
    Returns (hidden_new [n, ld] or None, a_s_next [n, ap] or None)."""
    n, ld = agg.shape
    hidden = torch.empty_like(agg) if want_hidden else None
    a_s = torch.empty((n, ap), dtype=torch.float32, device=agg.device) if Ws_next is not None else None
    c = lambda t: None if t is None else t.detach().contiguous()
    W_h, w_ih, w_hh, b_ih, b_hh = c(W_h), c(gate.weight_ih_l0), c(gate.weight_hh_l0), c(gate.bias_ih_l0), c(gate.bias_hh_l0)
    Ws_next, W_final = c(Ws_next), c(W_final)
    scratch = dense_scratch(d, precision, agg.device)
    ev = None
    if DENSE_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(_lib.lib().rg_dense_fwd(n, d, ld, _lib.ptr(agg), _lib.ptr(hidden_prev), _lib.ptr(prev_idx), _lib.ptr(W_h),
                                       {"idd": 0, "relu": 1, "tanh": 2}[act], _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(b_ih),
                                       _lib.ptr(b_hh), _lib.ptr(Ws_next), attn_dim, ap, _lib.ptr(a_s), _lib.ptr(W_final),
                                       _lib.ptr(nodes), n_ent, _lib.ptr(scores_all), _lib.ptr(hidden), DENSE_PRECISIONS[precision],
                                       _lib.ptr(scratch), 0 if scratch is None else scratch.numel(), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        DENSE_EVENTS.append((ev[0], ev[1], n))
    return hidden, a_s


def dense_fwd_dev(n_cap, count_ptr, agg, hidden_prev, prev_idx, d, W_h, act, gate, hidden_out, Ws_next=None, attn_dim=0, ap=0,
                  a_s_out=None, W_final=None, nodes=None, n_ent=0, scores_all=None, n_hint=0, precision="f32", scratch=None):
    """rg_dense_fwd_dev: the fused dense epilogue with the row count read on the device (buffers of capacity n_cap)."""
    ld = agg.shape[1]
    c = lambda t: None if t is None else t.detach().contiguous()
    W_h, w_ih, w_hh, b_ih, b_hh = c(W_h), c(gate.weight_ih_l0), c(gate.weight_hh_l0), c(gate.bias_ih_l0), c(gate.bias_hh_l0)
    Ws_next, W_final = c(Ws_next), c(W_final)
    if scratch is None:
        scratch = dense_scratch(d, precision, agg.device)
    _lib.check(_lib.lib().rg_dense_fwd_dev(n_cap, count_ptr, int(n_hint), d, ld, _lib.ptr(agg), _lib.ptr(hidden_prev), _lib.ptr(prev_idx),
                                           _lib.ptr(W_h), {"idd": 0, "relu": 1, "tanh": 2}[act], _lib.ptr(w_ih), _lib.ptr(w_hh),
                                           _lib.ptr(b_ih), _lib.ptr(b_hh), _lib.ptr(Ws_next), attn_dim, ap, _lib.ptr(a_s_out),
                                           _lib.ptr(W_final), _lib.ptr(nodes), n_ent, _lib.ptr(scores_all), _lib.ptr(hidden_out),
                                           DENSE_PRECISIONS[precision], _lib.ptr(scratch), 0 if scratch is None else scratch.numel(),
                                           _lib.stream_ptr()))


def dense_train_supported(d, act):
    return ((16 <= d <= 64 and d % 4 == 0) or d == 128) and act in ("idd", "relu", "tanh")


def dense_train_fwd(agg, hidden_prev, prev_idx, W_h, act, gate, mask=None, Ws_next=None):
    """rg_dense_train_fwd: (hidden_new [n,d], x [n,d], gates workspace [n,5d]) for the training step's dense part; with Ws_next
    [attn, d] (attn <= 16) also a_s [n, ap] = hidden_new Ws_next^T, the next layer's hoisted attention projection
    (rg_dense_train_fwd_as), as a fourth element (None without Ws_next)."""
    n, d = agg.shape
    dev = agg.device
    hidden = torch.empty((n, d), dtype=torch.float32, device=dev)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    ws = torch.empty((n, 5 * d), dtype=torch.float32, device=dev)
    c = lambda t: None if t is None else t.detach().contiguous()
    common = (n, d, _lib.ptr(c(agg)), _lib.ptr(c(hidden_prev)), _lib.ptr(prev_idx), _lib.ptr(c(W_h)),
              {"idd": 0, "relu": 1, "tanh": 2}[act], _lib.ptr(c(gate.weight_ih_l0)), _lib.ptr(c(gate.weight_hh_l0)),
              _lib.ptr(c(gate.bias_ih_l0)), _lib.ptr(c(gate.bias_hh_l0)), _lib.ptr(c(mask)))
    if Ws_next is None:
        _lib.check(_lib.lib().rg_dense_train_fwd(*common, _lib.ptr(hidden), _lib.ptr(x), _lib.ptr(ws), _lib.stream_ptr()))
        return hidden, x, ws, None
    attn = Ws_next.shape[0]
    ap = (attn + 3) // 4 * 4
    a_s = torch.empty((n, ap), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().rg_dense_train_fwd_as(*common, _lib.ptr(c(Ws_next)), attn, ap, _lib.ptr(hidden), _lib.ptr(x), _lib.ptr(ws),
                                                _lib.ptr(a_s), _lib.stream_ptr()))
    return hidden, x, ws, a_s


def rows_addmm(base, g, W):
    """base + g @ W for node-row matrices base [N, n], g [N, k] (k <= 32; rows may be spaced, unit-stride columns), W [k, n]: one HIP
    pass (rg_rows_addmm).  Returns a new [N, n] tensor."""
    assert base.is_cuda and base.dtype == g.dtype == W.dtype == torch.float32 and base.stride(1) == 1 and g.stride(1) == 1
    n_rows, n = base.shape
    k = W.shape[0]
    assert g.shape[0] == n_rows and g.shape[1] >= k and W.shape[1] == n
    out = torch.empty((n_rows, n), dtype=torch.float32, device=base.device)
    Wc = W.detach().contiguous()
    _lib.check(_lib.lib().rg_rows_addmm(C.c_void_p(base.data_ptr()), base.stride(0), C.c_void_p(g.data_ptr()), g.stride(0), k, _lib.ptr(Wc), n,
                                        n_rows, _lib.ptr(out), n, _lib.stream_ptr()))
    return out


def rows_linear(x, weight, bias=None):
    """F.linear(x, weight, bias) for node-row matrices x [N, k] (rows may be spaced, unit-stride columns) by rg_rows_linear: every
    output element is one fmaf chain over k in order, so a row's result does not depend on N.  No autograd.  Returns [N, n]."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    w = weight.detach().to(torch.float32).contiguous()
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    n_rows, k = x.shape
    n = w.shape[0]
    assert w.shape == (n, k) and (b is None or b.numel() == n)
    out = torch.empty((n_rows, n), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().rg_rows_linear(_lib.ptr(x), n_rows, x.stride(0), k, _lib.ptr(w), _lib.ptr(b), n, _lib.ptr(out), n,
                                         _lib.stream_ptr()))
    return out


def dense_train_bwd2(g_h, ws, x, mask, keep, act, W_h, w_ih, w_hh, prev_idx, n_old):
    """rg_dense_train_bwd2: (dgi [n,3d], dgh_n [n,d], dpre [n,d], dagg [n,d], g_prev [n_old,d]) - the hidden-side gate gradients as their
    n block only (r and z blocks = dgi's) and the carried state's gradient scattered to the previous frontier's rows by prev_idx."""
    n, d = x.shape
    dev = x.device
    f = lambda rows, cols: torch.empty((rows, cols), dtype=torch.float32, device=dev)
    dgi, dgh_n, dpre, dagg, g_prev = f(n, 3 * d), f(n, d), f(n, d), f(n, d), f(n_old, d)
    c = lambda t: None if t is None else t.detach().contiguous()
    _lib.check(_lib.lib().rg_dense_train_bwd2(n, d, _lib.ptr(c(g_h)), _lib.ptr(ws), _lib.ptr(x), _lib.ptr(c(mask)), float(keep),
                                              {"idd": 0, "relu": 1, "tanh": 2}[act], _lib.ptr(c(W_h)), _lib.ptr(c(w_ih)), _lib.ptr(c(w_hh)),
                                              _lib.ptr(prev_idx), _lib.ptr(dgi), _lib.ptr(dgh_n), _lib.ptr(dpre), _lib.ptr(dagg), _lib.ptr(g_prev),
                                              _lib.stream_ptr()))
    return dgi, dgh_n, dpre, dagg, g_prev


def dense_train_bwd_supported(d):
    return 16 <= d <= 64 and d % 4 == 0


def dense_train_bwd(g_h, ws, x, mask, keep, act, W_h, w_ih, w_hh):
    """rg_dense_train_bwd: (dgi [n,3d], dgh [n,3d], dpre [n,d], dagg [n,d], dh0 [n,d])."""
    n, d = x.shape
    dev = x.device
    f = lambda cols: torch.empty((n, cols), dtype=torch.float32, device=dev)
    dgi, dgh, dpre, dagg, dh0 = f(3 * d), f(3 * d), f(d), f(d), f(d)
    c = lambda t: None if t is None else t.detach().contiguous()
    _lib.check(_lib.lib().rg_dense_train_bwd(n, d, _lib.ptr(c(g_h)), _lib.ptr(ws), _lib.ptr(x), _lib.ptr(c(mask)), float(keep),
                                             {"idd": 0, "relu": 1, "tanh": 2}[act], _lib.ptr(c(W_h)), _lib.ptr(c(w_ih)), _lib.ptr(c(w_hh)),
                                             _lib.ptr(dgi), _lib.ptr(dgh), _lib.ptr(dpre), _lib.ptr(dagg), _lib.ptr(dh0), _lib.stream_ptr()))
    return dgi, dgh, dpre, dagg, dh0


def attn_tables(layers, q_rel, d, ld, attn_dim, ap):
    """Hoisted attention tables of all layers in ONE launch (rg_attn_tables): [(a_r [2R+1, ap], a_q [B, ap], rela padded to ld)] per layer.
    ``layers``: the GNNLayer modules (rela_embed, Wr_attn, Wqr_attn read in place: no stacking copies)."""
    L, dev = len(layers), q_rel.device
    n_rows, B = layers[0].rela_embed.weight.shape[0], q_rel.numel()
    a_r = torch.empty((L, n_rows, ap), dtype=torch.float32, device=dev)
    a_q = torch.empty((L, B, ap), dtype=torch.float32, device=dev)
    rela_p = torch.empty((L, n_rows, ld), dtype=torch.float32, device=dev) if ld != d else None
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    for l in layers:
        for t in (l.rela_embed.weight, l.Wr_attn.weight, l.Wqr_attn.weight, l.Wqr_attn.bias):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
    assert q_rel.dtype == torch.int64 and q_rel.is_contiguous()
    _lib.check(_lib.lib().rg_attn_tables(L, n_rows, B, d, ld, attn_dim, ap, arr([l.rela_embed.weight for l in layers]),
                                         arr([l.Wr_attn.weight for l in layers]), arr([l.Wqr_attn.weight for l in layers]),
                                         arr([l.Wqr_attn.bias for l in layers]), _lib.ptr(q_rel), _lib.ptr(a_r), _lib.ptr(a_q),
                                         _lib.ptr(rela_p), _lib.stream_ptr()))
    return [(a_r[i], a_q[i], rela_p[i] if rela_p is not None else layers[i].rela_embed.weight) for i in range(L)]


def rank(scores, ans_ptr, ans_idx, filt_ptr, filt_idx):
    """Filtered ranks (rg_rank) of every answer, fp32 [len(ans_idx)] in (query, answer) order."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous()
    B, n_ent = scores.shape
    out = torch.empty(ans_idx.numel(), dtype=torch.float32, device=scores.device)
    _lib.check(_lib.lib().rg_rank(_lib.ptr(scores), B, n_ent, _lib.ptr(ans_ptr), _lib.ptr(ans_idx),
                                  _lib.ptr(filt_ptr), _lib.ptr(filt_idx), _lib.ptr(out), _lib.stream_ptr()))
    return out


def topk(scores, k, q_key=None, known=None):
    """Filtered top-k (rg_topk) of every row of scores fp32 [B, n_ent]: (ids int32 [B, k], scores fp32 [B, k]), score descending then
    id ascending, -1 / -inf past the row's remaining entities.  ``known`` = (keys int64, ptr int64, idx int32) device tensors of a
    known-answer index (load_data.DataLoader.known_index) and ``q_key`` int64 [B] the rows' keys; None excludes nothing."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 2
    B, n_ent = scores.shape
    idx = torch.empty((B, k), dtype=torch.int32, device=scores.device)
    val = torch.empty((B, k), dtype=torch.float32, device=scores.device)
    if known is None or known[0].numel() == 0:
        keys = ptr = tails = q_key = None
        n_keys = 0
    else:
        keys, ptr, tails = known
        assert q_key is not None and q_key.dtype == torch.int64 and q_key.is_contiguous() and q_key.numel() == B
        assert keys.dtype == torch.int64 and ptr.dtype == torch.int64 and tails.dtype == torch.int32
        assert all(t.is_cuda and t.is_contiguous() for t in (q_key, keys, ptr, tails)) and ptr.numel() == keys.numel() + 1
        n_keys = keys.numel()
    _lib.check(_lib.lib().rg_topk(_lib.ptr(scores), B, n_ent, int(k), _lib.ptr(q_key), _lib.ptr(keys), _lib.ptr(ptr), _lib.ptr(tails),
                                  n_keys, _lib.ptr(idx), _lib.ptr(val), _lib.stream_ptr()))
    return idx, val


def _known_args(known, q_key, batch, who):
    """(q_key, keys, ptr, idx, n_keys) of a known-object index for the library: None / an empty index is n_keys = 0 with NULL arrays."""
    if known is None or known[0].numel() == 0:
        return None, None, None, None, 0
    keys, ptr, idx = known
    assert q_key is not None and q_key.dtype == torch.int64 and q_key.is_contiguous() and q_key.numel() == batch, who
    assert keys.dtype == torch.int64 and ptr.dtype == torch.int64 and idx.dtype == torch.int32, who
    assert all(t.is_cuda and t.is_contiguous() for t in (q_key, keys, ptr, idx)) and ptr.numel() == keys.numel() + 1, who
    return q_key, keys, ptr, idx, keys.numel()


def segment_rank(scores, ent, seg_ptr, target, key_sp=None, known_sp=None, key_spt=None, known_spt=None):
    """Raw, (s, p)-filtered and (s, p, t)-filtered ranks (rg_segment_rank) of every query's target among ITS visited entities:
    (rank, rank_fil, rank_fil_t fp32 [B], found int32 [B]).  ``scores`` fp32 [N] and ``ent`` int32 [N] per visited pair, query q owning
    seg_ptr[q]:seg_ptr[q+1] (int32 or int64 [B+1]); ``target`` int32 [B]; ``known_*`` = (keys int64, ptr int64, idx int32) device
    tensors with the rows' keys ``key_*`` int64 [B], None filtering nothing.  Unfound targets: found 0, ranks 1e9."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 1
    assert ent.is_cuda and ent.dtype == torch.int32 and ent.is_contiguous() and ent.shape == scores.shape
    assert target.is_cuda and target.dtype == torch.int32 and target.is_contiguous() and target.dim() == 1
    B = target.numel()
    assert seg_ptr.is_cuda and seg_ptr.dtype in (torch.int32, torch.int64) and seg_ptr.is_contiguous() and seg_ptr.numel() == B + 1
    dev = scores.device
    rank, rank_fil, rank_fil_t = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
    found = torch.empty(B, dtype=torch.int32, device=dev)
    sp, spt = _known_args(known_sp, key_sp, B, "segment_rank: (s, p) index"), _known_args(known_spt, key_spt, B, "segment_rank: (s, p, t) index")
    p = _lib.ptr
    _lib.check(_lib.lib().rg_segment_rank(p(scores), p(ent), scores.numel(), p(seg_ptr), int(seg_ptr.dtype == torch.int64), p(target), B,
                                          p(sp[0]), p(sp[1]), p(sp[2]), p(sp[3]), sp[4], p(spt[0]), p(spt[1]), p(spt[2]), p(spt[3]), spt[4],
                                          p(rank), p(rank_fil), p(rank_fil_t), p(found), _lib.stream_ptr()))
    return rank, rank_fil, rank_fil_t, found


def segment_eval(scores, ent, seg_ptr, target, n_ent, key_a=None, known_a=None, key_b=None, known_b=None):
    """Loss term and rank counts (rg_segment_eval) of every query's target on ITS dense score row - the visited pairs plus an exact
    0 for each of the other n_ent - n_seg entities - without building it: (logp fp32 [B], counts int32 [B, 6], visited int32 [B]).
    logp = log(softmax(row)[target] + 1e-12); counts = (gt, eq) over every entity, over those the list of ``known_a`` keeps and over
    those the list of ``known_b`` keeps (the target always kept, never its own tie); visited = 1 where the target has a pair.
    ``scores`` (logits) fp32 [N], ``ent`` int32 [N], ``seg_ptr`` int32 or int64 [B+1], ``target`` int32 [B] and the two indexes with
    their per-query keys as segment_rank."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 1
    assert ent.is_cuda and ent.dtype == torch.int32 and ent.is_contiguous() and ent.shape == scores.shape
    assert target.is_cuda and target.dtype == torch.int32 and target.is_contiguous() and target.dim() == 1
    B = target.numel()
    assert seg_ptr.is_cuda and seg_ptr.dtype in (torch.int32, torch.int64) and seg_ptr.is_contiguous() and seg_ptr.numel() == B + 1
    dev = scores.device
    logp = torch.empty(B, dtype=torch.float32, device=dev)
    counts = torch.empty((B, 6), dtype=torch.int32, device=dev)
    visited = torch.empty(B, dtype=torch.int32, device=dev)
    ka, kb = _known_args(known_a, key_a, B, "segment_eval: first index"), _known_args(known_b, key_b, B, "segment_eval: second index")
    p = _lib.ptr
    _lib.check(_lib.lib().rg_segment_eval(p(scores), p(ent), scores.numel(), p(seg_ptr), int(seg_ptr.dtype == torch.int64), p(target), B,
                                          int(n_ent), p(ka[0]), p(ka[1]), p(ka[2]), p(ka[3]), ka[4], p(kb[0]), p(kb[1]), p(kb[2]), p(kb[3]),
                                          kb[4], p(logp), p(counts), p(visited), _lib.stream_ptr()))
    return logp, counts, visited


SEGMENT_TOPK_STAGE_MAX = 24576       # csrc/segment_topk.hip: SEG_STAGE_MAX (longer segments are re-read on every pass of the select)
SEGMENT_TOPK_LIST_LDS = 256          # ... SEG_LIST_LDS (longer known lists are searched in memory)


def segment_topk(scores, ent, seg_ptr, k, q_key=None, known=None, want_prob=True):
    """Filtered top-k (rg_segment_topk) of every query's segment of visited pairs: (ids int32 [B, k], scores fp32 [B, k], prob fp32
    [B, k] or None), score descending then entity id ascending, -1 / -inf / 0 past the query's kept pairs.  ``scores`` (logits) fp32
    [N], ``ent`` int32 [N] and ``seg_ptr`` int32 or int64 [B+1] as segment_rank; ``known`` = (keys int64, ptr int64, idx int32) device
    tensors with the queries' keys ``q_key`` int64 [B], None excluding nothing.  prob: the per-query softmax over the whole segment."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 1
    assert ent.is_cuda and ent.dtype == torch.int32 and ent.is_contiguous() and ent.shape == scores.shape
    assert seg_ptr.is_cuda and seg_ptr.dtype in (torch.int32, torch.int64) and seg_ptr.is_contiguous() and seg_ptr.dim() == 1
    B = seg_ptr.numel() - 1
    dev = scores.device
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    val = torch.empty((B, k), dtype=torch.float32, device=dev)
    prob = torch.empty((B, k), dtype=torch.float32, device=dev) if want_prob else None
    kn = _known_args(known, q_key, B, "segment_topk: known-object index")
    p = _lib.ptr
    _lib.check(_lib.lib().rg_segment_topk(p(scores), p(ent), scores.numel(), p(seg_ptr), int(seg_ptr.dtype == torch.int64), B, int(k),
                                          p(kn[0]), p(kn[1]), p(kn[2]), p(kn[3]), kn[4], p(idx), p(val), p(prob), _lib.stream_ptr()))
    return idx, val, prob


PATHS_MAX_K = 8                      # csrc/paths.hip: PATHS_MAX_K
PATHS_SCRATCH_BYTES = 256 << 20      # default scratch budget of paths_topk


def paths_scratch_bytes(n_edges, k):
    return int(_lib.lib().rg_paths_scratch_bytes(int(n_edges), int(k)))


def paths_topk(edges, alpha, offsets, n_hops, k, scratch_bytes=PATHS_SCRATCH_BYTES, offsets_host=None):
    """The k best paths (rg_paths_topk) of every row of a compact r-digraph: (edge int64 [B, k, L] indices into ``edges``, -1 past
    the row's count; product float64 [B, k], 0 past it; count int32 [B]).  ``edges`` int32 [E, 5], ``alpha`` fp32 [E], ``offsets``
    int64 [B+1] (validated by the caller: non-decreasing, ending at E; ``offsets_host``: its copy as a numpy array, if at hand).
    The rows are walked in chunks whose scratch stays within ``scratch_bytes`` (one row at least per chunk); rows are independent,
    so the chunking changes no bit of the result."""
    assert edges.is_cuda and edges.dtype == torch.int32 and edges.is_contiguous() and edges.dim() == 2 and edges.shape[1] == 5
    assert alpha.is_cuda and alpha.dtype == torch.float32 and alpha.is_contiguous() and alpha.shape == (edges.shape[0],)
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.dim() == 1
    B, L, dev = offsets.numel() - 1, int(n_hops), edges.device
    path_edge = torch.full((B, k, L), -1, dtype=torch.int64, device=dev)
    path_prod = torch.zeros((B, k), dtype=torch.float64, device=dev)
    path_count = torch.zeros(B, dtype=torch.int32, device=dev)
    if B == 0 or edges.shape[0] == 0:
        return path_edge, path_prod, path_count
    off = offsets.cpu().numpy() if offsets_host is None else offsets_host
    chunks, lo = [], 0
    while lo < B:                    # the longest run of rows from lo whose edges fit the budget
        hi = lo + 1
        while hi < B and 0 < paths_scratch_bytes(off[hi + 1] - off[lo], k) <= scratch_bytes:
            hi += 1
        chunks.append((lo, hi))
        lo = hi
    need = [paths_scratch_bytes(off[hi] - off[lo], k) for lo, hi in chunks]
    if min(need) == 0:
        raise ValueError("paths_topk: a chunk of %d edges is beyond the kernel's 2^31 edge indices"
                         % max(off[hi] - off[lo] for lo, hi in chunks))
    scratch = torch.empty(max(need), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    for lo, hi in chunks:
        _lib.check(_lib.lib().rg_paths_topk(p(edges), p(alpha), p(offsets), lo, hi, L, int(k), p(scratch), p(path_edge), p(path_prod),
                                            p(path_count), _lib.stream_ptr()))
    return path_edge, path_prod, path_count


DIGRAPH_CHUNK = 128                  # include/redgnn.h: RG_DIGRAPH_CHUNK

DIGRAPH_EVENTS = None                # probes: a list that collects (start, end, n_dst, n_edges) of every digraph_(t)layer_fwd


def digraph_chunks(dst_ptr_host):
    """(cut destinations, chunks they make, longest destination) of a hop's CSR (numpy int [n_dst + 1]): a destination of more than
    DIGRAPH_CHUNK edges is cut into chunks of that many, summed by separate waves."""
    length = np.diff(np.asarray(dst_ptr_host, np.int64))
    hub = length > DIGRAPH_CHUNK
    return int(hub.sum()), int(((length[hub] + DIGRAPH_CHUNK - 1) // DIGRAPH_CHUNK).sum()), int(length.max()) if length.size else 0


def digraph_layer_fwd(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, want_alpha=True,
                      dst_ptr_host=None):
    """One message-passing layer over an explicit, destination-segmented edge list (rg_digraph_layer_fwd): (agg fp32 [n_dst, ld], alpha
    fp32 [E] or None).  ``dst_ptr`` int32 [n_dst + 1] is the CSR of the hop's edges by destination, ``src_idx`` / ``rel`` int32 [E] an
    edge's row in ``hidden`` / ``a_s`` and in ``rela`` / ``a_r``, ``row_of_dst`` int32 [n_dst] a destination's row in ``a_q``
    (``dst_ptr_host``: the CSR as a numpy array, if at hand).  Shapes, dtypes and index ranges are checked here (ValueError); the sums
    are deterministic and a destination's row does not depend on the rest of the call."""
    return _digraph_layer("digraph_layer_fwd", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha,
                          attn_dim, want_alpha, dst_ptr_host, None)


def digraph_tlayer_fwd(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, time_tab, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, edge_time,
                       q_time, n_dir=3, want_alpha=True, dst_ptr_host=None):
    """digraph_layer_fwd with a time per edge (rg_digraph_tlayer_fwd): ``edge_time`` int32 [E], ``q_time`` int32 [B] (a row of ``a_q``
    each) and ``time_tab`` fp32 [n_dir * n_time, ld].  n_dir = 3, the interpolation layer: ``hidden`` [3 n_src, ld] and ``rela``
    [3 n_rela_rows, ld] hold a row per direction past / now / future of dt = edge time - query time, ``time_tab`` a row per direction
    and |dt|, and ``edge_time`` lies in 0..n_time-1.  n_dir = 1, the extrapolation form: plain tables, ``time_tab`` is read at
    clamp(query day - edge day, 0, n_time - 1) and ``edge_time`` >= 0 is the day the caller resolved for the edge.  ``a_s`` [n_src, ap]
    and ``a_r`` [n_rela_rows, ap] are not directed.  The same checks (ValueError), the same determinism."""
    return _digraph_layer("digraph_tlayer_fwd", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha,
                          attn_dim, want_alpha, dst_ptr_host, (edge_time, q_time, time_tab, n_dir))


def digraph_layer_fwd_gated(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, t, gate_lo=None,
                            gate_hi=None, want_alpha=True, dst_ptr_host=None, check_index=True):
    """digraph_layer_fwd with a gate on every edge's message, for ``t.numel()`` replicas of the hop in one launch
    (rg_digraph_layer_fwd_gated): (agg fp32 [n_rep * n_dst, ld], alpha fp32 [n_rep * E] or None).  ``t`` fp32 [n_rep]; ``gate_lo`` /
    ``gate_hi`` fp32 [E] in the order of the edge list, or None for 0 / 1; replica k's gate is fmaf(t[k], hi - lo, lo), it reads rows
    k * n_src + s of ``hidden`` [n_rep * n_src, ld] and ``a_s`` [n_rep * n_src, ap] and writes rows k * n_dst + o of agg; the index arrays
    and the other tables are shared.  The gate multiplies the message and does not enter alpha; at gate 1 the bits are
    digraph_layer_fwd's, and a replica's are those of a one-replica call with its t.  digraph_layer_fwd's checks (ValueError);
    ``check_index`` False skips the range check of the index arrays (a caller that hands over the same arrays again)."""
    return _digraph_layer("digraph_layer_fwd_gated", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha,
                          attn_dim, want_alpha, dst_ptr_host, None, (t, gate_lo, gate_hi), check_index)


def digraph_layer_fwd_gates(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, gate,
                            want_alpha=True, dst_ptr_host=None, check_index=True):
    """digraph_layer_fwd_gated with a gate per (replica, edge) (rg_digraph_layer_fwd_gates): ``gate`` fp32 [n_rep, E] in the order of
    the edge list, replica k's gates its row k, taken as they are.  The stacked arguments and results of digraph_layer_fwd_gated;
    replica k's bits are those of a one-replica digraph_layer_fwd_gated call with gate_lo = gate_hi = gate[k] and t = 1."""
    return _digraph_layer("digraph_layer_fwd_gates", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha,
                          attn_dim, want_alpha, dst_ptr_host, None, (gate,), check_index)


def _check_gates(who, gated, E, n_rows):
    """(n_rep, t, gate_lo, gate_hi) of a gated wrapper: ``t`` fp32 [n_rep] with n_rep >= 1 dividing the ``n_rows`` rows of the stacked
    state, ``gate_lo`` / ``gate_hi`` fp32 [E] or None.  ``gated`` of one entry is the per-replica form, (n_rep, gate): ``gate`` fp32
    [n_rep, E] with n_rep >= 1 dividing ``n_rows``."""
    if len(gated) == 1:
        gate, = gated
        if not (torch.is_tensor(gate) and gate.dtype == torch.float32 and gate.dim() == 2 and gate.shape[0] >= 1 and gate.shape[1] == E):
            raise ValueError("%s: gate must be float32 [n_rep, %d], a row per replica (at least one) and an entry per edge" % (who, E))
        if n_rows % gate.shape[0]:
            raise ValueError("%s: the %d rows of hidden and a_s are not a whole number of rows for each of the %d replicas"
                             % (who, n_rows, gate.shape[0]))
        return gate.shape[0], gate
    t, lo, hi = gated
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() >= 1):
        raise ValueError("%s: t must be a float32 vector with an entry per replica (at least one)" % who)
    for name, g in (("gate_lo", lo), ("gate_hi", hi)):
        if g is not None and not (torch.is_tensor(g) and g.dtype == torch.float32 and tuple(g.shape) == (E,)):
            raise ValueError("%s: %s must be float32 [%d], one per edge, or None" % (who, name, E))
    if n_rows % t.numel():
        raise ValueError("%s: the %d rows of hidden and a_s are not a whole number of rows for each of the %d replicas" % (who, n_rows, t.numel()))
    return t.numel(), t, lo, hi


def _digraph_layer(who, dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, want_alpha,
                   dst_ptr_host, timed, gated=None, check_index=True):
    """Every forward wrapper: the host checks, the scratch, the launch.  ``timed``: None or (edge_time, q_time, time_tab, n_dir);
    ``gated``: None, (t, gate_lo, gate_hi) or (gate [n_rep, E],), static only."""
    ints, floats = [("dst_ptr", dst_ptr), ("src_idx", src_idx), ("rel", rel), ("row_of_dst", row_of_dst)], \
        [("hidden", hidden), ("rela", rela), ("a_s", a_s), ("a_r", a_r), ("a_q", a_q)]
    n_dir = 1
    if timed is not None:
        edge_time, q_time, time_tab, n_dir = timed
        if isinstance(n_dir, (bool, np.bool_)) or not isinstance(n_dir, (int, np.integer)) or n_dir not in (1, 3):
            raise ValueError("%s: n_dir must be 1 or 3 (got %r)" % (who, n_dir))
        ints += [("edge_time", edge_time), ("q_time", q_time)]
        floats.append(("time_tab", time_tab))
    for name, t in ints:
        if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 1):
            raise ValueError("%s: %s must be an int32 vector" % (who, name))
    for name, t in floats:
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2):
            raise ValueError("%s: %s must be a float32 matrix" % (who, name))
    n_dst, E = dst_ptr.numel() - 1, src_idx.numel()
    ld, ap = hidden.shape[1], a_s.shape[1]
    n_rep, gates = 1, ()
    if gated is not None:
        n_rep, *gates = _check_gates(who, gated, E, a_s.shape[0])
    n_src = a_s.shape[0] // n_rep
    if n_dst < 0 or rel.numel() != E or row_of_dst.numel() != n_dst:
        raise ValueError("%s: dst_ptr [%d], src_idx [%d], rel [%d] and row_of_dst [%d] do not fit together"
                         % (who, dst_ptr.numel(), E, rel.numel(), row_of_dst.numel()))
    if rela.shape[1] != ld or a_r.shape[1] != ap or a_q.shape[1] != ap or n_dir * a_s.shape[0] != hidden.shape[0] \
            or n_dir * a_r.shape[0] != rela.shape[0]:
        raise ValueError("%s: hidden %s, rela %s, a_s %s, a_r %s and a_q %s do not fit together"
                         % (who, tuple(hidden.shape), tuple(rela.shape), tuple(a_s.shape), tuple(a_r.shape), tuple(a_q.shape)))
    n_time = 0
    if timed is not None:
        n_time = time_tab.shape[0] // n_dir
        if edge_time.numel() != E or q_time.numel() != a_q.shape[0] or time_tab.shape[1] != ld or n_time < 1 or n_time * n_dir != time_tab.shape[0]:
            raise ValueError("%s: edge_time [%d] (%d edges), q_time [%d] (a_q %s) and time_tab %s (n_dir * n_time rows of %d) do not fit together"
                             % (who, edge_time.numel(), E, q_time.numel(), tuple(a_q.shape), tuple(time_tab.shape), ld))
    _require_gpu(hidden.device)
    tensors = tuple(t for _, t in ints + floats) + (w_alpha, b_alpha) + tuple(g for g in gates if g is not None)
    if not all(t.is_cuda and t.is_contiguous() for t in tensors):
        raise ValueError("%s: every tensor must be contiguous and on the device" % who)
    dev = hidden.device
    agg = torch.zeros((n_rep * max(n_dst, 0), ld), dtype=torch.float32, device=dev)
    alpha = torch.zeros(n_rep * E, dtype=torch.float32, device=dev) if want_alpha else None
    ptr_h = np.ascontiguousarray(dst_ptr.cpu().numpy() if dst_ptr_host is None else dst_ptr_host, dtype=np.int32)
    if ptr_h.shape != (n_dst + 1,) or ptr_h[0] != 0 or ptr_h[-1] != E or (np.diff(ptr_h) < 0).any():
        raise ValueError("%s: dst_ptr must start at 0, never decrease and end at the number of edges (%d)" % (who, E))
    if E and check_index:
        checked = [("src_idx", src_idx, n_src), ("rel", rel, a_r.shape[0]), ("row_of_dst", row_of_dst, a_q.shape[0])]
        if timed is not None:                 # n_dir 3: a time id; n_dir 1: a day, any that is not negative
            checked.append(("edge_time", edge_time, n_time if n_dir == 3 else 1 << 31))
        lo = torch.stack([t.min() for _, t, _ in checked]).tolist()
        hi = torch.stack([t.max() for _, t, _ in checked]).tolist()
        for (name, _, n), a, b in zip(checked, lo, hi):
            if a < 0 or b >= n:
                raise ValueError("%s: %s out of range (%d..%d, %d rows)" % (who, name, a, b, n))
    L, p = _lib.lib(), _lib.ptr
    if n_dst <= 0:
        nbytes = 0
    elif gated is not None:
        nbytes = int(L.rg_digraph_layer_fwd_gated_scratch_bytes(p(ptr_h), n_dst, ld, n_rep))
    else:
        nbytes = int(L.rg_digraph_layer_fwd_scratch_bytes(p(ptr_h), n_dst, ld))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    ev = None
    if DIGRAPH_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    if gated is not None and len(gates) == 1:
        _lib.check(L.rg_digraph_layer_fwd_gates(n_rep, p(gates[0]), n_dst, E, p(dst_ptr), p(ptr_h), p(src_idx), p(rel), p(row_of_dst), n_src,
                                                a_r.shape[0], a_q.shape[0], p(hidden), p(rela), int(d), ld, p(a_s), p(a_r), p(a_q), ap,
                                                p(w_alpha), p(b_alpha), int(attn_dim), p(agg), p(alpha), p(scratch), nbytes,
                                                _lib.stream_ptr()))
    elif gated is not None:
        _lib.check(L.rg_digraph_layer_fwd_gated(n_rep, p(gates[0]), p(gates[1]), p(gates[2]), n_dst, E, p(dst_ptr), p(ptr_h), p(src_idx), p(rel),
                                                p(row_of_dst), n_src, a_r.shape[0], a_q.shape[0], p(hidden), p(rela), int(d), ld, p(a_s), p(a_r),
                                                p(a_q), ap, p(w_alpha), p(b_alpha), int(attn_dim), p(agg), p(alpha), p(scratch), nbytes,
                                                _lib.stream_ptr()))
    elif timed is None:
        _lib.check(L.rg_digraph_layer_fwd(n_dst, E, p(dst_ptr), p(ptr_h), p(src_idx), p(rel), p(row_of_dst), a_s.shape[0], a_r.shape[0],
                                          a_q.shape[0], p(hidden), p(rela), int(d), ld, p(a_s), p(a_r), p(a_q), ap, p(w_alpha), p(b_alpha),
                                          int(attn_dim), p(agg), p(alpha), p(scratch), nbytes, _lib.stream_ptr()))
    else:
        _lib.check(L.rg_digraph_tlayer_fwd(n_dst, E, p(dst_ptr), p(ptr_h), p(src_idx), p(rel), p(edge_time), p(row_of_dst), p(q_time),
                                           a_s.shape[0], a_r.shape[0], a_q.shape[0], n_time, int(n_dir), p(hidden), p(rela), p(time_tab),
                                           int(d), ld, p(a_s), p(a_r), p(a_q), ap, p(w_alpha), p(b_alpha), int(attn_dim), p(agg), p(alpha),
                                           p(scratch), nbytes, _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        DIGRAPH_EVENTS.append((ev[0], ev[1], n_rep * n_dst, n_rep * E))
    return agg, alpha


DIGRAPH_BWD_EVENTS = None            # probes: a list that collects (start, end, n_src, n_edges) of every digraph_layer_bwd


def digraph_source_view(dst_ptr, src_idx, n_src, key=None):
    """The source-segmented view of a hop rg_digraph_layer_bwd sums over, from the destination-ordered lists digraph_layer_fwd takes:
    (src_ptr int32 [n_src + 1], src_ptr_host numpy, edge_of int32 [E], dst_of_edge int32 [E]).  ``edge_of`` is the stable sort of the
    edges by source, so a source's edges keep their list order; ``dst_of_edge[e]`` is the destination whose CSR row holds e.
    ``key`` (an integer vector [E] with values in 0 .. n_src - 1): segment by it instead of by ``src_idx`` - the directed source row
    of rg_digraph_tlayer_bwd, ``n_src`` then counting those rows (digraph_directed_rows)."""
    key = src_idx if key is None else key
    E, dev = key.numel(), key.device
    edge_of = torch.sort(key, stable=True).indices.to(torch.int32)
    src_ptr = torch.zeros(n_src + 1, dtype=torch.int64, device=dev)
    if E:
        src_ptr[1:] = torch.cumsum(torch.bincount(key, minlength=n_src)[:n_src], 0)
    src_ptr = src_ptr.to(torch.int32)
    n_dst = dst_ptr.numel() - 1
    dst_of_edge = torch.repeat_interleave(torch.arange(n_dst, dtype=torch.int32, device=dev), (dst_ptr[1:] - dst_ptr[:-1]).long(),
                                          output_size=E)
    return src_ptr, src_ptr.cpu().numpy(), edge_of.contiguous(), dst_of_edge.contiguous()


def digraph_directed_rows(dst_ptr, src_idx, row_of_dst, edge_time, q_time, n_dir):
    """int64 [E]: the directed source row u of every edge of a timed hop, the row of ``hidden`` rg_digraph_tlayer_fwd reads for it -
    u = 3 s + dir with dir = 0 / 1 / 2 for edge time - query time < 0 / == 0 / > 0 (64-bit differences) for n_dir = 3, u = s for
    n_dir = 1."""
    if n_dir == 1:
        return src_idx.long()
    n_dst, E = dst_ptr.numel() - 1, src_idx.numel()
    dst_of_edge = torch.repeat_interleave(torch.arange(n_dst, device=src_idx.device), (dst_ptr[1:] - dst_ptr[:-1]).long(), output_size=E)
    dt = edge_time.long() - q_time.long()[row_of_dst.long()[dst_of_edge]]
    return 3 * src_idx.long() + torch.sign(dt) + 1


def digraph_layer_bwd(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg,
                      want_state=True):
    """The adjoint of digraph_layer_fwd on the same arguments with respect to a gate on every edge's message, ``hidden`` and ``a_s``
    (rg_digraph_layer_bwd; ``rela``, ``a_r``, ``a_q``, ``w_alpha`` and ``b_alpha`` are constants): (grad_gate fp32 [E] in the order of
    the edge list, grad_hidden fp32 [n_src, ld], grad_a_s fp32 [n_src, ap]) for ``grad_agg`` fp32 [n_dst, ld]; the last two are None
    with ``want_state`` False (hop 1: the state is the constant 0), grad_gate's bits unchanged.  The source-segmented view of the hop
    is built here (digraph_source_view).  The same checks as digraph_layer_fwd (ValueError); no float atomics, the same bits on every
    run, and a source's rows and its edges' gate gradients do not depend on the rest of the call."""
    return _digraph_layer_bwd("digraph_layer_bwd", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha,
                              attn_dim, grad_agg, want_state, None)


def digraph_tlayer_bwd(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, time_tab, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg,
                       edge_time, q_time, n_dir=3, want_state=True):
    """The adjoint of digraph_tlayer_fwd on the same arguments with respect to a gate on every edge's message, ``hidden`` and ``a_s``
    (rg_digraph_tlayer_bwd; the tables, ``a_r``, ``a_q``, ``w_alpha`` and ``b_alpha`` are constants): (grad_gate fp32 [E] in the order
    of the edge list, grad_hidden fp32 [n_dir * n_src, ld] by directed row, grad_a_s fp32 [n_src, ap]) for ``grad_agg`` fp32 [n_dst,
    ld]; the last two are None with ``want_state`` False (hop 1: the state is the constant 0), grad_gate's bits unchanged.  The kernel
    works on directed source rows (digraph_directed_rows); the view segmented by them is built here, and a source's three attention
    rows are added in the fixed order past, now, future.  digraph_tlayer_fwd's checks (ValueError); no float atomics, the same bits
    on every run."""
    return _digraph_layer_bwd("digraph_tlayer_bwd", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha,
                              attn_dim, grad_agg, want_state, (edge_time, q_time, time_tab, n_dir))


def digraph_layer_bwd_gated(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg, t,
                            gate_lo=None, gate_hi=None, want_state=True, view=None, check_index=True):
    """The adjoint of digraph_layer_fwd_gated on the same arguments (rg_digraph_layer_bwd_gated): (grad_gate fp32 [n_rep * E], replica k's
    at k * E + the edge's list position, grad_hidden fp32 [n_rep * n_src, ld], grad_a_s fp32 [n_rep * n_src, ap]) for ``grad_agg`` fp32
    [n_rep * n_dst, ld]; grad_gate is the derivative with respect to the gate itself at the gate fmaf(t[k], hi - lo, lo).  At gate 1 the
    bits are digraph_layer_bwd's, and a replica's are those of a one-replica call with its t.  ``view``: the hop's
    digraph_source_view, if at hand (it does not depend on the gates or the replicas); ``check_index`` as the forward's."""
    return _digraph_layer_bwd("digraph_layer_bwd_gated", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha,
                              b_alpha, attn_dim, grad_agg, want_state, None, (t, gate_lo, gate_hi), view, check_index)


def digraph_layer_bwd_gates(dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg, gate,
                            want_state=True, view=None, check_index=True):
    """The adjoint of digraph_layer_fwd_gates on the same arguments (rg_digraph_layer_bwd_gates): digraph_layer_bwd_gated's stacked
    results at the gates ``gate`` fp32 [n_rep, E]; replica k's bits are those of a one-replica digraph_layer_bwd_gated call with
    gate_lo = gate_hi = gate[k] and t = 1."""
    return _digraph_layer_bwd("digraph_layer_bwd_gates", dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha,
                              b_alpha, attn_dim, grad_agg, want_state, None, (gate,), view, check_index)


MASK_CHUNK = 512                     # include/redgnn.h: RG_MASK_CHUNK


def mask_step(offsets, free, score, target, inv_scale, inv_n, lambda_size, lambda_ent, grad, theta, m, v, step, lr=0.05, beta1=0.9,
              beta2=0.999, eps=1e-8, gate_out=None):
    """One step of learning an edge mask for R replicas of a digraph's E edges (rg_mask_step; see include/redgnn.h for the
    arithmetic): ``theta``, ``m``, ``v`` fp32 [R, E] are updated IN PLACE on the free edges (``free`` uint8 or bool [E]) and
    (gate_out fp32 [R, E], size fp32 [R, B], count int32 [R, B]) is returned - the new gates (``gate_out``, if given, is written on
    the free edges and otherwise left as it is; None: a new array of zeros), their sum over a row's free edges and how many of them
    are above 0.5.  ``offsets`` int64 [B + 1] the digraph's, ``score`` fp32 [R, B], ``target`` / ``inv_scale`` / ``inv_n`` fp32 [B],
    ``lambda_size`` / ``lambda_ent`` fp32 [R], ``grad`` fp32 [R, E] = d score / d gate, ``step`` >= 1 Adam's step count.  Shapes and
    dtypes are checked here (ValueError).  No float atomics: the same bits on every run, and a replica's do not depend on the
    others."""
    who = "mask_step"
    if isinstance(step, (bool, np.bool_)) or not isinstance(step, (int, np.integer)) or step < 1:
        raise ValueError("%s: step must be a count from 1 (got %r)" % (who, step))
    if not (torch.is_tensor(theta) and theta.dtype == torch.float32 and theta.dim() == 2 and theta.shape[0] >= 1):
        raise ValueError("%s: theta must be float32 [R, E] with at least one replica" % who)
    R, E = theta.shape
    if not (torch.is_tensor(offsets) and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 1):
        raise ValueError("%s: offsets must be int64 [B + 1]" % who)
    B = offsets.numel() - 1
    if torch.is_tensor(free) and free.dtype == torch.bool:
        free = free.view(torch.uint8)
    if not (torch.is_tensor(free) and free.dtype == torch.uint8 and tuple(free.shape) == (E,)):
        raise ValueError("%s: free must be uint8 or bool [%d], one per edge" % (who, E))
    if gate_out is None:
        gate_out = torch.zeros((R, E), dtype=torch.float32, device=theta.device)
    for name, x, shape in (("m", m, (R, E)), ("v", v, (R, E)), ("grad", grad, (R, E)), ("gate_out", gate_out, (R, E)), ("score", score, (R, B)),
                           ("target", target, (B,)), ("inv_scale", inv_scale, (B,)), ("inv_n", inv_n, (B,)),
                           ("lambda_size", lambda_size, (R,)), ("lambda_ent", lambda_ent, (R,))):
        if not (torch.is_tensor(x) and x.dtype == torch.float32 and tuple(x.shape) == shape):
            raise ValueError("%s: %s must be float32 %s" % (who, name, list(shape)))
    _require_gpu(theta.device)
    tensors = (offsets, free, score, target, inv_scale, inv_n, lambda_size, lambda_ent, grad, theta, m, v, gate_out)
    if not all(x.is_cuda and x.is_contiguous() for x in tensors):
        raise ValueError("%s: every tensor must be contiguous and on the device" % who)
    size = torch.zeros((R, B), dtype=torch.float32, device=theta.device)
    count = torch.zeros((R, B), dtype=torch.int32, device=theta.device)
    p = _lib.ptr
    _lib.check(_lib.lib().rg_mask_step(R, B, E, p(offsets), p(free), p(score), p(target), p(inv_scale), p(inv_n), p(lambda_size),
                                       p(lambda_ent), p(grad), float(lr), float(beta1), float(beta2), float(eps), int(step), p(theta), p(m),
                                       p(v), p(gate_out), p(size), p(count), _lib.stream_ptr()))
    return gate_out, size, count


MASK_TIE_CHUNK = 32                  # include/redgnn.h: RG_MASK_TIE_CHUNK


def mask_tie_grad(grp_ptr, member, grad, n_groups, grp_ptr_host=None):
    """The chain rule through tied gates (rg_mask_tie_grad; see include/redgnn.h for the sum's definition): grp_grad fp32 [R, n_groups],
    entry (k, g) the sum of ``grad`` fp32 [R, E] over the edges member[grp_ptr[g] : grp_ptr[g + 1]] of group g, added in member order
    in chunks of MASK_TIE_CHUNK, the chunk sums in chunk order; +0 for an empty group.  ``grp_ptr`` int32 [n_groups + 1] (starting at
    0, never decreasing, ending at member.numel(); ``grp_ptr_host``: the same array as numpy, if at hand), ``member`` int32 [M] edge
    positions (clamped into 0 .. E - 1).  Shapes and dtypes are checked here (ValueError).  No float atomics: the same bits on every
    run, and a (replica, group) sum does not depend on the others."""
    who = "mask_tie_grad"
    if isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer)) or n_groups < 0:
        raise ValueError("%s: n_groups must be a count >= 0 (got %r)" % (who, n_groups))
    n_groups = int(n_groups)
    if not (torch.is_tensor(grad) and grad.dtype == torch.float32 and grad.dim() == 2 and grad.shape[0] >= 1):
        raise ValueError("%s: grad must be float32 [R, E] with at least one replica" % who)
    R, E = grad.shape
    if not (torch.is_tensor(grp_ptr) and grp_ptr.dtype == torch.int32 and tuple(grp_ptr.shape) == (n_groups + 1,)):
        raise ValueError("%s: grp_ptr must be int32 [%d], n_groups + 1" % (who, n_groups + 1))
    if not (torch.is_tensor(member) and member.dtype == torch.int32 and member.dim() == 1):
        raise ValueError("%s: member must be int32 [M]" % who)
    M = member.numel()
    ptr_h = np.ascontiguousarray(grp_ptr.cpu().numpy() if grp_ptr_host is None else grp_ptr_host, dtype=np.int32)
    if ptr_h.shape != (n_groups + 1,) or ptr_h[0] != 0 or ptr_h[-1] != M:     # (that it never decreases: the entry point's one pass)
        raise ValueError("%s: grp_ptr must start at 0, never decrease and end at the number of members (%d)" % (who, M))
    if M and not E:
        raise ValueError("%s: %d members but grad has no edges" % (who, M))
    _require_gpu(grad.device)
    if not all(x.is_cuda and x.is_contiguous() for x in (grp_ptr, member, grad)):
        raise ValueError("%s: every tensor must be contiguous and on the device" % who)
    if n_groups == 0 or M == 0:                                               # no sum to form: every group is empty
        return torch.zeros((R, n_groups), dtype=torch.float32, device=grad.device)
    grp_grad = torch.empty((R, n_groups), dtype=torch.float32, device=grad.device)    # every cell is written: an empty group's with +0
    L, p = _lib.lib(), _lib.ptr
    nbytes = int(L.rg_mask_tie_grad_scratch_bytes(p(ptr_h), n_groups, R))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=grad.device) if nbytes else None
    _lib.check(L.rg_mask_tie_grad(R, E, n_groups, M, p(grp_ptr), p(ptr_h), p(member), p(grad), p(grp_grad), p(scratch), nbytes,
                                  _lib.stream_ptr()))
    return grp_grad


def mask_tie_gates(group_of, grp_gate, gate_out):
    """Tied gates written back to the edges (rg_mask_tie_gates): gate_out[k, e] = grp_gate[k, group_of[e]] where group_of[e] >= 0, IN
    PLACE; every other cell of ``gate_out`` fp32 [R, E] is left as it is.  ``group_of`` int32 [E] (-1: not tied; clamped to
    n_groups - 1), ``grp_gate`` fp32 [R, n_groups].  Returns ``gate_out``.  Shapes and dtypes are checked here (ValueError)."""
    who = "mask_tie_gates"
    if not (torch.is_tensor(gate_out) and gate_out.dtype == torch.float32 and gate_out.dim() == 2 and gate_out.shape[0] >= 1):
        raise ValueError("%s: gate_out must be float32 [R, E] with at least one replica" % who)
    R, E = gate_out.shape
    if not (torch.is_tensor(group_of) and group_of.dtype == torch.int32 and tuple(group_of.shape) == (E,)):
        raise ValueError("%s: group_of must be int32 [%d], one per edge" % (who, E))
    if not (torch.is_tensor(grp_gate) and grp_gate.dtype == torch.float32 and grp_gate.dim() == 2 and grp_gate.shape[0] == R):
        raise ValueError("%s: grp_gate must be float32 [%d, n_groups]" % (who, R))
    _require_gpu(gate_out.device)
    if not all(x.is_cuda and x.is_contiguous() for x in (group_of, grp_gate, gate_out)):
        raise ValueError("%s: every tensor must be contiguous and on the device" % who)
    if E == 0 or grp_gate.shape[1] == 0:                                      # no gate to hand on
        return gate_out
    p = _lib.ptr
    _lib.check(_lib.lib().rg_mask_tie_gates(R, E, grp_gate.shape[1], p(group_of), p(grp_gate), p(gate_out), _lib.stream_ptr()))
    return gate_out


def _digraph_layer_bwd(who, dst_ptr, src_idx, rel, row_of_dst, hidden, rela, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg,
                       want_state, timed, gated=None, view=None, check_index=True):
    """Every backward wrapper: the host checks, the source view, the scratch, the launch.  ``timed``: None or (edge_time, q_time,
    time_tab, n_dir); ``gated``: None, (t, gate_lo, gate_hi) or (gate [n_rep, E],), static only."""
    ints = [("dst_ptr", dst_ptr), ("src_idx", src_idx), ("rel", rel), ("row_of_dst", row_of_dst)]
    floats = [("hidden", hidden), ("rela", rela), ("a_s", a_s), ("a_r", a_r), ("a_q", a_q), ("grad_agg", grad_agg)]
    n_dir = 1
    if timed is not None:
        edge_time, q_time, time_tab, n_dir = timed
        if isinstance(n_dir, (bool, np.bool_)) or not isinstance(n_dir, (int, np.integer)) or n_dir not in (1, 3):
            raise ValueError("%s: n_dir must be 1 or 3 (got %r)" % (who, n_dir))
        n_dir = int(n_dir)
        ints += [("edge_time", edge_time), ("q_time", q_time)]
        floats.append(("time_tab", time_tab))
    for name, t in ints:
        if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 1):
            raise ValueError("%s: %s must be an int32 vector" % (who, name))
    for name, t in floats:
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2):
            raise ValueError("%s: %s must be a float32 matrix" % (who, name))
    n_dst, E = dst_ptr.numel() - 1, src_idx.numel()
    ld, ap = hidden.shape[1], a_s.shape[1]
    n_rep, gates = 1, ()
    if gated is not None:
        n_rep, *gates = _check_gates(who, gated, E, a_s.shape[0])
    n_src = a_s.shape[0] // n_rep
    n_rows = n_dir * n_src                                # the rows of hidden, of the source view and of the state outputs (per replica)
    if n_dst < 0 or rel.numel() != E or row_of_dst.numel() != n_dst:
        raise ValueError("%s: dst_ptr [%d], src_idx [%d], rel [%d] and row_of_dst [%d] do not fit together"
                         % (who, dst_ptr.numel(), E, rel.numel(), row_of_dst.numel()))
    if rela.shape[1] != ld or a_r.shape[1] != ap or a_q.shape[1] != ap or hidden.shape[0] != n_rep * n_rows or n_dir * a_r.shape[0] != rela.shape[0] \
            or tuple(grad_agg.shape) != (n_rep * n_dst, ld):
        raise ValueError("%s: hidden %s, rela %s, a_s %s, a_r %s, a_q %s and grad_agg %s (%d destinations) do not fit together"
                         % (who, tuple(hidden.shape), tuple(rela.shape), tuple(a_s.shape), tuple(a_r.shape), tuple(a_q.shape),
                            tuple(grad_agg.shape), n_dst))
    n_time = 0
    if timed is not None:
        n_time = time_tab.shape[0] // n_dir
        if edge_time.numel() != E or q_time.numel() != a_q.shape[0] or time_tab.shape[1] != ld or n_time < 1 or n_time * n_dir != time_tab.shape[0]:
            raise ValueError("%s: edge_time [%d] (%d edges), q_time [%d] (a_q %s) and time_tab %s (n_dir * n_time rows of %d) do not fit together"
                             % (who, edge_time.numel(), E, q_time.numel(), tuple(a_q.shape), tuple(time_tab.shape), ld))
    _require_gpu(hidden.device)
    tensors = tuple(t for _, t in ints + floats) + (w_alpha, b_alpha) + tuple(g for g in gates if g is not None)
    if not all(t.is_cuda and t.is_contiguous() for t in tensors):
        raise ValueError("%s: every tensor must be contiguous and on the device" % who)
    dev = hidden.device
    grad_gate = torch.zeros(n_rep * E, dtype=torch.float32, device=dev)
    grad_hidden = torch.zeros((n_rep * n_rows, ld), dtype=torch.float32, device=dev) if want_state else None
    grad_a_s = torch.zeros((n_rep * n_rows, ap), dtype=torch.float32, device=dev) if want_state else None
    ptr_h = dst_ptr.cpu().numpy() if check_index else None
    if check_index and (ptr_h[0] != 0 or ptr_h[-1] != E or (np.diff(ptr_h) < 0).any()):
        raise ValueError("%s: dst_ptr must start at 0, never decrease and end at the number of edges (%d)" % (who, E))
    if E and check_index:
        checked = [("src_idx", src_idx, n_src), ("rel", rel, a_r.shape[0]), ("row_of_dst", row_of_dst, a_q.shape[0])]
        if timed is not None:                 # n_dir 3: a time id; n_dir 1: a day, any that is not negative
            checked.append(("edge_time", edge_time, n_time if n_dir == 3 else 1 << 31))
        lo = torch.stack([t.min() for _, t, _ in checked]).tolist()
        hi = torch.stack([t.max() for _, t, _ in checked]).tolist()
        for (name, _, n), a, b in zip(checked, lo, hi):
            if a < 0 or b >= n:
                raise ValueError("%s: %s out of range (%d..%d, %d rows)" % (who, name, a, b, n))
    key = None if timed is None else digraph_directed_rows(dst_ptr, src_idx, row_of_dst, edge_time, q_time, n_dir)
    src_ptr, src_ptr_h, edge_of, dst_of_edge = digraph_source_view(dst_ptr, src_idx, n_rows, key=key) if view is None else view
    if src_ptr.numel() != n_rows + 1 or edge_of.numel() != E or dst_of_edge.numel() != E:
        raise ValueError("%s: view is not the source view of this hop (%d sources, %d edges)" % (who, n_rows, E))
    L, p = _lib.lib(), _lib.ptr
    if n_rows <= 0:
        nbytes = 0
    elif gated is not None:
        nbytes = int(L.rg_digraph_layer_bwd_gated_scratch_bytes(p(src_ptr_h), n_rows, ld, ap, n_rep))
    else:
        nbytes = int(L.rg_digraph_layer_bwd_scratch_bytes(p(src_ptr_h), n_rows, ld, ap))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    ev = None
    if DIGRAPH_BWD_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    if gated is not None and len(gates) == 1:
        _lib.check(L.rg_digraph_layer_bwd_gates(n_rep, p(gates[0]), n_src, n_dst, E, p(src_ptr), p(src_ptr_h), p(edge_of), p(dst_of_edge),
                                                p(rel), p(row_of_dst), a_r.shape[0], a_q.shape[0], p(hidden), p(rela), int(d), ld, p(a_s),
                                                p(a_r), p(a_q), ap, p(w_alpha), p(b_alpha), int(attn_dim), p(grad_agg), p(grad_gate),
                                                p(grad_hidden), p(grad_a_s), p(scratch), nbytes, _lib.stream_ptr()))
    elif gated is not None:
        _lib.check(L.rg_digraph_layer_bwd_gated(n_rep, p(gates[0]), p(gates[1]), p(gates[2]), n_src, n_dst, E, p(src_ptr), p(src_ptr_h),
                                                p(edge_of), p(dst_of_edge), p(rel), p(row_of_dst), a_r.shape[0], a_q.shape[0], p(hidden),
                                                p(rela), int(d), ld, p(a_s), p(a_r), p(a_q), ap, p(w_alpha), p(b_alpha), int(attn_dim),
                                                p(grad_agg), p(grad_gate), p(grad_hidden), p(grad_a_s), p(scratch), nbytes,
                                                _lib.stream_ptr()))
    elif timed is None:
        _lib.check(L.rg_digraph_layer_bwd(n_src, n_dst, E, p(src_ptr), p(src_ptr_h), p(edge_of), p(dst_of_edge), p(rel), p(row_of_dst),
                                          a_r.shape[0], a_q.shape[0], p(hidden), p(rela), int(d), ld, p(a_s), p(a_r), p(a_q), ap, p(w_alpha),
                                          p(b_alpha), int(attn_dim), p(grad_agg), p(grad_gate), p(grad_hidden), p(grad_a_s), p(scratch), nbytes,
                                          _lib.stream_ptr()))
    else:
        _lib.check(L.rg_digraph_tlayer_bwd(n_src, n_dst, E, p(src_ptr), p(src_ptr_h), p(edge_of), p(dst_of_edge), p(rel), p(edge_time),
                                           p(row_of_dst), p(q_time), a_r.shape[0], a_q.shape[0], n_time, n_dir, p(hidden), p(rela),
                                           p(time_tab), int(d), ld, p(a_s), p(a_r), p(a_q), ap, p(w_alpha), p(b_alpha), int(attn_dim),
                                           p(grad_agg), p(grad_gate), p(grad_hidden), p(grad_a_s), p(scratch), nbytes, _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        DIGRAPH_BWD_EVENTS.append((ev[0], ev[1], n_rep * n_rows, n_rep * E))
    if want_state and n_dir == 3:             # a source's three rows: past, now, future, added in that order
        g = grad_a_s.view(n_src, 3, ap)
        grad_a_s = ((g[:, 0] + g[:, 1]) + g[:, 2]).contiguous()
    return grad_gate, grad_hidden, grad_a_s


# include/redgnn.h: RG_DIGRAPH_INDEX_*, with the ValueError each status bit becomes ({who}, {L} filled in by digraph_index_error)
DIGRAPH_INDEX_STATUS = (
    (4, "{who}: edges hold a row that is not the row of its range in offsets, or hops that are not 1..{L} in order inside a row"),
    (8, "{who}: edges hold a head or tail out of range (n_ent={n_ent})"),
    (16, "{who}: edges hold a relation out of range ({n_rela_rows} relation rows)"),
    (1, "{who}: edges must be ordered by (row, hop, tail), as model.explain returns them"),
    (2, "{who}: the hop-{L} edges of a row must share their tail, the row's answer"),
)

DIGRAPH_INDEX_EVENTS = None          # probes: a list that collects (start, end, hop, n_hop_edges) of every digraph_hop_index


def digraph_index_error(status, who, L, n_ent, n_rela_rows):
    """The ValueError of a non-zero status word of digraph_hop_ranges / digraph_hop_index (the first of DIGRAPH_INDEX_STATUS that is set: an edge in the wrong place
    or out of range comes before what follows from it), or None."""
    for bit, text in DIGRAPH_INDEX_STATUS:
        if status & bit:
            return ValueError(text.format(who=who, L=L, n_ent=n_ent, n_rela_rows=n_rela_rows))
    return None


def _check_digraph_edges(who, edges):
    if not (torch.is_tensor(edges) and edges.dtype == torch.int32 and edges.dim() == 2 and edges.shape[1] == 5):
        raise ValueError("%s: edges must be int32 [E, 5]" % who)
    if edges.shape[0] >= 1 << 31:
        raise ValueError("%s: %d edges are beyond the kernels' 2^31 edge indices" % (who, edges.shape[0]))


class DigraphHopRanges:
    """digraph_hop_ranges: hop_ptr int64 [B, L + 1] and hop_first int32 [L, B + 1] on the device, hop_ptr_host (numpy, the former's
    copy), hop_edges (list of L ints: the edges of every hop) and the status word (0: in order)."""

    def __init__(self, hop_ptr, hop_first, hop_ptr_host, hop_edges, status):
        self.hop_ptr, self.hop_first, self.hop_ptr_host, self.hop_edges, self.status = hop_ptr, hop_first, hop_ptr_host, hop_edges, status


def digraph_hop_ranges(edges, offsets, n_hops):
    """Where every hop of every row of a compact r-digraph lies (rg_digraph_hop_ranges): a DigraphHopRanges.  ``edges`` int32 [E, 5]
    ordered by (row, hop, tail) and ``offsets`` int64 [B + 1], device tensors (offsets validated by the caller: starting at 0, never
    decreasing, ending at E).  Once per digraph; every digraph_hop_index call then touches only its hop's edges."""
    who = "digraph_hop_ranges"
    _check_digraph_edges(who, edges)
    if not (torch.is_tensor(offsets) and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 1):
        raise ValueError("%s: offsets must be int64 [B + 1]" % who)
    if isinstance(n_hops, (bool, np.bool_)) or not isinstance(n_hops, (int, np.integer)) or not 1 <= n_hops <= 32:
        raise ValueError("%s: n_hops must be an integer in 1..32 (got %r)" % (who, n_hops))
    _require_gpu(edges.device)
    if not (edges.is_cuda and offsets.is_cuda and edges.is_contiguous() and offsets.is_contiguous() and offsets.device == edges.device):
        raise ValueError("%s: edges and offsets must be contiguous and on one device" % who)
    E, B, L, dev = edges.shape[0], offsets.numel() - 1, int(n_hops), edges.device
    hop_ptr = torch.zeros((B, L + 1), dtype=torch.int64, device=dev)
    hop_first = torch.zeros((L, B + 1), dtype=torch.int32, device=dev)
    ptr_h, n_h, status = np.zeros((B, L + 1), np.int64), np.zeros(L, np.int64), C.c_int32(0)
    p = _lib.ptr
    _lib.check(_lib.lib().rg_digraph_hop_ranges(p(edges), p(offsets), E, B, L, p(hop_ptr), p(hop_first), p(ptr_h), p(n_h),
                                                C.byref(status), _lib.stream_ptr()))
    return DigraphHopRanges(hop_ptr, hop_first, ptr_h, [int(x) for x in n_h], int(status.value))


def digraph_hop_index(edges, ranges, hop, keys_prev, n_ent, n_rela_rows, live, keep=None, edge_time=None):
    """The index of hop ``hop`` of a rescore (rg_digraph_hop_index): (at int32 [n_live], src int32 [n_live], rel int32 [n_live], time
    int32 [n_live] or None, keys int64 [n_dst], dst_ptr int32 [n_dst + 1], row_of int32 [n_dst], prev_idx int32 [n_dst], status int) -
    explain._hop_index's arrays for the same inputs, with the relation and the time of every live edge gathered along.  ``ranges``:
    digraph_hop_ranges of the same edges; ``keys_prev`` int64, sorted and unique, row * n_ent + entity; ``keep`` uint8 [E] or None;
    ``edge_time`` int32 [E] or None; ``live`` uint8 [E] receives live[at] = 1.  status != 0 (digraph_index_error): the edges of the hop
    are malformed and the arrays mean nothing.  No live edge: empty arrays, and nothing else of the hop is read back."""
    who = "digraph_hop_index"
    if not isinstance(ranges, DigraphHopRanges):
        raise ValueError("%s: ranges must be digraph_hop_ranges' result" % who)
    B, L = ranges.hop_ptr.shape[0], ranges.hop_ptr.shape[1] - 1
    _check_digraph_edges(who, edges)
    if isinstance(hop, (bool, np.bool_)) or not isinstance(hop, (int, np.integer)) or not 1 <= hop <= L:
        raise ValueError("%s: hop must be an integer in 1..%d (got %r)" % (who, L, hop))
    for name, x in (("n_ent", n_ent), ("n_rela_rows", n_rela_rows)):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 1 <= x < 1 << 31:
            raise ValueError("%s: %s must be a positive integer (got %r)" % (who, name, x))
    E, dev = edges.shape[0], edges.device
    if not (torch.is_tensor(keys_prev) and keys_prev.dtype == torch.int64 and keys_prev.dim() == 1):
        raise ValueError("%s: keys_prev must be an int64 vector" % who)
    if not (torch.is_tensor(live) and live.dtype == torch.uint8 and live.shape == (E,)):
        raise ValueError("%s: live must be uint8 [%d], one per edge" % (who, E))
    if keep is not None and not (torch.is_tensor(keep) and keep.dtype == torch.uint8 and keep.shape == (E,)):
        raise ValueError("%s: keep must be uint8 [%d], one per edge, or None" % (who, E))
    if edge_time is not None and not (torch.is_tensor(edge_time) and edge_time.dtype == torch.int32 and edge_time.shape == (E,)):
        raise ValueError("%s: edge_time must be int32 [%d], one per edge, or None" % (who, E))
    _require_gpu(dev)
    tensors = [edges, keys_prev, live, ranges.hop_ptr, ranges.hop_first] + [t for t in (keep, edge_time) if t is not None]
    if not all(t.is_cuda and t.is_contiguous() and t.device == dev for t in tensors):
        raise ValueError("%s: every tensor must be contiguous and on one device" % who)
    n_hop = ranges.hop_edges[hop - 1]
    if n_hop > E:
        raise ValueError("%s: the ranges are another digraph's (%d edges in hop %d, %d in all)" % (who, n_hop, hop, E))
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    at, src, rel, tm = i32(n_hop), i32(n_hop), i32(n_hop), (i32(n_hop) if edge_time is not None else None)
    keys, dst_ptr, row_of, prev_idx = torch.empty(n_hop, dtype=torch.int64, device=dev), i32(n_hop + 1), i32(n_hop), i32(n_hop)
    L_, p = _lib.lib(), _lib.ptr
    nbytes = int(L_.rg_digraph_hop_index_scratch_bytes(n_hop))
    scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev) if nbytes else None
    scr_p = None if scratch is None else C.c_void_p((scratch.data_ptr() + 255) // 256 * 256)
    n_live, n_dst, status = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    ev = None
    if DIGRAPH_INDEX_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(L_.rg_digraph_hop_index(p(edges), p(keep), p(edge_time), E, B, L, int(hop), p(ranges.hop_ptr), p(ranges.hop_first[hop - 1]),
                                       n_hop, p(keys_prev), keys_prev.numel(), int(n_ent), int(n_rela_rows), p(at), p(src), p(rel), p(tm),
                                       p(keys), p(dst_ptr), p(row_of), p(prev_idx), p(live), scr_p, nbytes, C.byref(n_live),
                                       C.byref(n_dst), C.byref(status), _lib.stream_ptr()))
    if ev is not None:
        ev[1].record()
        DIGRAPH_INDEX_EVENTS.append((ev[0], ev[1], int(hop), n_hop))
    nl, nd = int(n_live.value), int(n_dst.value)
    return (at[:nl], src[:nl], rel[:nl], None if tm is None else tm[:nl], keys[:nd], dst_ptr[:nd + 1] if nl else dst_ptr[:0], row_of[:nd],
            prev_idx[:nd], int(status.value))


RULE_MAX_HOPS = 32                  # csrc/rule_bits.h: RULE_MAX_HOPS
RULE_MAX_RULES = 65535               # ... RULE_MAX_RULES (rules of one call)
RULE_SCRATCH_BYTES = 1 << 30         # default scratch budget of rule_ground
# tools/probe_rule_quality.py sets this to a list to collect (start_event, end_event, n_rules, n_sources) per chunk of rule_ground
RULE_EVENTS = None


def rule_ground_scratch_bytes(n_ent, n_rules, n_sources):
    return int(_lib.lib().rg_rule_ground_scratch_bytes(int(n_ent), int(n_rules), int(n_sources)))


def _int_array(x, name, who):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.dtype not in (np.int32, np.int64):
        raise ValueError("%s: %s must be int32 or int64 (got %s)" % (who, name, a.dtype))
    return a


def _as32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _check_scratch_bytes(scratch_bytes, who):
    if isinstance(scratch_bytes, (bool, np.bool_)) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < 0:
        raise ValueError("%s: scratch_bytes must be a non-negative integer (got %r)" % (who, scratch_bytes))
    return int(scratch_bytes)


def _check_rule_shapes(who, h, b, **steps):
    """head [R], body and every array of ``steps`` (named as the caller's arguments) [R, L] with 1 <= L <= RULE_MAX_HOPS, or ValueError."""
    if h.ndim != 1 or b.ndim != 2 or b.shape[0] != h.shape[0] or any(x.shape != b.shape for x in steps.values()):
        names, shapes = ["body"] + list(steps), [str(x.shape) for x in (h, b) + tuple(steps.values())]
        want = "head must be [R], %s and %s [R, L]" % (", ".join(names[:-1]), names[-1]) if steps else "head must be [R] and body [R, L]"
        raise ValueError("%s: %s (got %s and %s)" % (who, want, ", ".join(shapes[:-1]), shapes[-1]))
    if not 1 <= b.shape[1] <= RULE_MAX_HOPS:
        raise ValueError("%s: the body length %d is not in 1..%d" % (who, b.shape[1], RULE_MAX_HOPS))


def _check_rel_range(who, h, b, top, note=""):
    """Every relation id of head and body in 0..top, or ValueError (``note``: what top is, inside the bracket)."""
    if h.size and (min(h.min(), b.min()) < 0 or max(h.max(), b.max()) > top):
        raise ValueError("%s: relation id out of range 0..%d (%sgot %d..%d)"
                         % (who, top, note, min(h.min(), b.min()), max(h.max(), b.max())))


def _check_anchors(who, anchors, n_ent, n_unit, unit):
    """int64 [S, 2] = (entity, ``unit``: "time id" or "day", in 0..n_unit-1), distinct, sorted by (unit, entity), or ValueError."""
    a = _int_array(anchors, "anchors", who)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("%s: anchors must be [S, 2] = (entity, %s) (got %s)" % (who, unit, a.shape))
    a = a.astype(np.int64)
    if a.size and (a[:, 0].min() < 0 or a[:, 0].max() >= n_ent or a[:, 1].min() < 0 or a[:, 1].max() >= n_unit):
        raise ValueError("%s: anchor out of range (entity 0..%d, %s 0..%d; got %d..%d and %d..%d)"
                         % (who, n_ent - 1, unit, n_unit - 1, a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()))
    key = np.sort(a[:, 1] * n_ent + a[:, 0])
    if np.unique(key).size != key.size:
        raise ValueError("%s: duplicate anchors (%d pairs, %d distinct)" % (who, key.size, np.unique(key).size))
    return np.stack([key % n_ent, key // n_ent], 1)


def _check_heads_and_weights(who, h, weight):
    """weight as float32 [R], finite and in (0, 1], for rules whose heads ``h`` do not decrease, or ValueError."""
    if h.size > 1 and (np.diff(h) < 0).any():
        at = int(np.argmax(np.diff(h) < 0))
        raise ValueError("%s: head must be non-decreasing (rule %d has head %d after %d)" % (who, at + 1, h[at + 1], h[at]))
    w = weight.detach().cpu().numpy() if torch.is_tensor(weight) else np.asarray(weight)
    if w.dtype.kind != "f" or w.ndim != 1 or w.shape[0] != h.shape[0]:
        raise ValueError("%s: weight must be a float array [R] (got %s %s for %d rules)" % (who, w.dtype, w.shape, h.shape[0]))
    w = np.ascontiguousarray(w, dtype=np.float32)
    if w.size and not (np.isfinite(w).all() and (w > 0).all() and (w <= 1).all()):
        bad = int(np.argmax(~(np.isfinite(w) & (w > 0) & (w <= 1))))
        raise ValueError("%s: weights must be finite and in (0, 1] as float32 (rule %d has %r)" % (who, bad, float(w[bad])))
    return w


def check_rules(n_ent, n_rel, head, body, sources=None, who="rule_ground"):
    """The host validation of rule_ground: (head int32 [R], body int32 [R, L], sources int32 [S]) as contiguous numpy arrays, or
    ValueError.  ``sources=None``: every entity."""
    h, b = _int_array(head, "head", who), _int_array(body, "body", who)
    _check_rule_shapes(who, h, b)
    n_ent, n_rel = int(n_ent), int(n_rel)
    _check_rel_range(who, h, b, 2 * n_rel, "2*n_rel; ")
    if sources is None:
        s = np.arange(n_ent, dtype=np.int32)
    else:
        s = _int_array(sources, "sources", who)
        if s.ndim != 1:
            raise ValueError("%s: sources must be [S] (got %s)" % (who, s.shape))
        if s.size and (s.min() < 0 or s.max() >= n_ent):
            raise ValueError("%s: source id out of range 0..%d (got %d..%d)" % (who, n_ent - 1, s.min(), s.max()))
        if np.unique(s).size != s.size:
            raise ValueError("%s: duplicate sources (%d ids, %d distinct)" % (who, s.size, np.unique(s).size))
    return _as32(h), _as32(b), _as32(s)


def rule_chunking(n_ent, n_rules, n_sources, scratch_bytes):
    """(rules per chunk, sources per block) of rule_ground: all sources in one block if one rule's scratch fits the budget then, else
    the largest multiple of 32 that does (at least 32); then as many rules as fit (at least one)."""
    def fits(r, s):
        return 0 < rule_ground_scratch_bytes(n_ent, r, s) <= scratch_bytes

    def largest(hi, ok):             # the largest x in 1..hi with ok(x), ok being monotone; 1 if none
        lo = 1
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid - 1)
        return lo
    blocks = (n_sources + 31) // 32
    s_c = 32 * largest(blocks, lambda k: fits(1, 32 * k))
    n_r = largest(min(n_rules, RULE_MAX_RULES), lambda r: fits(r, s_c))
    if rule_ground_scratch_bytes(n_ent, n_r, s_c) == 0:
        raise ValueError("rule_ground: %d entities are beyond the bitmaps' range" % n_ent)
    return n_r, s_c


def rule_ground(graph, head, body, sources=None, scratch_bytes=RULE_SCRATCH_BYTES):
    """The four counts of every rule (head[i], body[i]) on ``graph`` (rg_rule_ground): int64 [R, 4] on the device = (body_pairs, hits,
    pca_body_pairs, head_pairs) over the pairs (x, y) with x in ``sources`` (distinct entity ids; None: every entity).  Relation ids
    are the graph's, 0..2*n_rel (inverses and the identity included).  Ids are validated on the host (ValueError).  The work is cut
    into chunks of (rules x source blocks of a multiple of 32) whose bitmaps fit ``scratch_bytes`` (one rule and 32 sources at least);
    the scratch is allocated once and the counts are integers added per chunk, so the result does not depend on the budget."""
    if getattr(graph, "n_time", 0):
        raise ValueError("rule_ground: temporal graph: rules are grounded on static and inductive graphs only "
                         "(temporal rules, whose steps carry a direction, are grounded by trule_ground)")
    scratch_bytes = _check_scratch_bytes(scratch_bytes, "rule_ground")
    h, b, s = check_rules(graph.n_ent, graph.n_rel, head, body, sources)
    L, p = b.shape[1], _lib.ptr

    def upload(dev, s_c):
        h_d, b_d, s_d = (torch.from_numpy(a).to(dev) for a in (h, b, s))
        return lambda r0, r1, k, s0, s1, scratch, counts: _lib.check(_lib.lib().rg_rule_ground(
            graph.handle, p(h_d[r0:r1]), p(b_d[r0:r1]), r1 - r0, L, p(s_d[s0:s1]), s1 - s0, p(scratch), p(counts), _lib.stream_ptr()))
    return _ground_chunks("RULE_EVENTS", graph, h.shape[0], s.shape[0], scratch_bytes, upload)


def _ground_chunks(events, graph, R, S, scratch_bytes, upload):
    """What rule_ground, trule_ground and xrule_ground do once their arguments are valid: int64 [R, 4] counts of R rules over S
    columns, the work cut as rule_chunking says.  ``upload(dev, s_c)`` puts the family's arrays on the device, knowing the columns of a
    block, and returns ``call(r0, r1, k, s0, s1, scratch, counts)``: the entry point on the rules r0..r1 and block k = columns s0..s1,
    adding into ``counts`` [r1 - r0, 4].  The scratch is allocated once, for the largest chunk.  ``events`` names the module attribute
    (RULE_EVENTS, ...) that collects a pair of events, the rules and the columns of every chunk where a probe has set it to a list."""
    dev = _require_gpu(graph.device)
    counts = torch.zeros((R, 4), dtype=torch.int64, device=dev)
    if R == 0 or S == 0:
        return counts
    n_r, s_c = rule_chunking(graph.n_ent, R, S, scratch_bytes)
    call = upload(dev, s_c)
    with torch.cuda.device(dev):
        scratch = torch.empty(rule_ground_scratch_bytes(graph.n_ent, min(n_r, R), min(s_c, S)), dtype=torch.uint8, device=dev)
        for r0 in range(0, R, n_r):
            r1 = min(r0 + n_r, R)
            for k, s0 in enumerate(range(0, S, s_c)):
                s1 = min(s0 + s_c, S)
                log = globals()[events]                  # read at call time: a test or probe assigns the attribute
                if log is not None:
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record()
                call(r0, r1, k, s0, s1, scratch, counts[r0:r1])
                if log is not None:
                    ev[1].record()
                    log.append((ev[0], ev[1], r1 - r0, s1 - s0))
    return counts


def _block_anchor_ptr(unit_of, n_unit, s_c):
    """int [blocks, n_unit + 1]: anchor_ptr of every block of ``s_c`` consecutive anchors, ``unit_of`` [S] being their sorted time ids
    (days): clip(ptr - s0, 0, s1 - s0), ptr[tau] the first anchor whose time is >= tau."""
    S = unit_of.shape[0]
    ptr = np.searchsorted(unit_of, np.arange(n_unit + 1))
    starts = np.arange(0, S, s_c)
    return np.clip(ptr[None, :] - starts[:, None], 0, np.minimum(starts + s_c, S)[:, None] - starts[:, None])


# tools/probe_trule_quality.py sets this to a list to collect (start_event, end_event, n_rules, n_anchors) per chunk of trule_ground
TRULE_EVENTS = None
TRULE_DIRECTIONS = ("past", "now", "future", "any")      # the step directions 0..3 of a temporal rule


def trule_ground_scratch_bytes(n_ent, n_rules, n_anchors):
    return int(_lib.lib().rg_trule_ground_scratch_bytes(int(n_ent), int(n_rules), int(n_anchors)))


def check_trules(graph, head, body, direction, anchors=None, who="trule_ground"):
    """The host validation of trule_ground: (head int32 [R], body int32 [R, L], direction int32 [R, L], anchors int64 [S, 2] =
    (entity, time id) sorted by (time, entity)) as contiguous numpy arrays, or ValueError.  ``graph`` needs n_ent, n_rela_rows and
    n_time (and default_anchors() where ``anchors`` is None); no device is touched."""
    n_time = int(getattr(graph, "n_time", 0) or 0)
    if n_time == 0:
        raise ValueError("%s: static graph (no time ids): static rules are grounded by rule_ground" % who)
    n_ent, n_rows = int(graph.n_ent), int(graph.n_rela_rows)
    h, b, d = _int_array(head, "head", who), _int_array(body, "body", who), _int_array(direction, "direction", who)
    _check_rule_shapes(who, h, b, direction=d)
    _check_rel_range(who, h, b, n_rows - 1)
    if d.size and (d.min() < 0 or d.max() > 3):
        raise ValueError("%s: direction out of range 0..3 (past, now, future, any; got %d..%d)" % (who, d.min(), d.max()))
    a = graph.default_anchors() if anchors is None else _check_anchors(who, anchors, n_ent, n_time, "time id")
    return _as32(h), _as32(b), _as32(d), a


def trule_ground(graph, head, body, direction, anchors=None, scratch_bytes=RULE_SCRATCH_BYTES):
    """The four counts of every temporal rule (head[i], (body[i], direction[i])) on the quadruple graph ``graph`` (rg_trule_ground;
    include/redgnn.h has the definition): int64 [R, 4] on the device = (body_pairs, hits, pca_body_pairs, head_pairs) over the pairs
    ((x, t), y) with (x, t) in ``anchors``, int [S, 2] = (entity, time id), distinct; None: graph.default_anchors().  Relation ids
    are the graph's, 0..n_rela_rows-1; directions 0 past, 1 now, 2 future (of the edge's time against the anchor's, as the forward
    forms it), 3 any.  Everything is validated on the host (ValueError).  The anchors are sorted by (time, entity) and the work is cut
    into chunks of (rules x blocks of consecutive anchors, a multiple of 32) whose bitmaps fit ``scratch_bytes``, as rule_chunking
    says; each block gets anchor_ptr = clip(ptr - s0, 0, s1 - s0), ptr being the first sorted anchor of every time id.  The scratch
    is allocated once and the counts are integers added per chunk, so the result does not depend on the budget."""
    scratch_bytes = _check_scratch_bytes(scratch_bytes, "trule_ground")
    h, b, d, a = check_trules(graph, head, body, direction, anchors)
    L, p = b.shape[1], _lib.ptr

    def upload(dev, s_c):
        h_d, b_d, d_d, e_d, p_d = (torch.from_numpy(_as32(x)).to(dev)
                                   for x in (h, b, d, a[:, 0], _block_anchor_ptr(a[:, 1], graph.n_time, s_c)))
        return lambda r0, r1, k, s0, s1, scratch, counts: _lib.check(_lib.lib().rg_trule_ground(
            graph.handle, p(h_d[r0:r1]), p(b_d[r0:r1]), p(d_d[r0:r1]), r1 - r0, L, p(e_d[s0:s1]), p(p_d[k]), s1 - s0, p(scratch),
            p(counts), _lib.stream_ptr()))
    return _ground_chunks("TRULE_EVENTS", graph, h.shape[0], a.shape[0], scratch_bytes, upload)


# tools/probe_xrule_quality.py sets this to a list to collect (start_event, end_event, n_rules, n_anchors) per chunk of xrule_ground
XRULE_EVENTS = None
XRULE_LOOP_WINDOW = 120              # extrapolation.WINDOW: the lag the forward gives the self-loop of a full window
XRULE_ANY_HI = 2 ** 31 - 1           # the open end of a lag range: [0, XRULE_ANY_HI) is "any lag"


def xrule_default_anchors(graph, row_day):
    """int64 [S, 2] = (entity, day) sorted by (day, entity): the distinct (subject, day) pairs of the data rows of an extrapolation
    graph (the rows whose time field, their data-row index, is below n_data = len(row_day)), read from the rows the graph was built
    from - the anchors xrule_ground counts over when given none."""
    rows = getattr(graph, "_rows", None)
    if rows is None or rows[1] is not None:
        raise ValueError("xrule_ground: the graph no longer holds its rows: pass anchors")
    q, day = rows[0], np.asarray(row_day, dtype=np.int64).reshape(-1)
    q = q[(q[:, 3] >= 0) & (q[:, 3] < len(day))]
    key = np.unique(day[q[:, 3]] * int(graph.n_ent) + q[:, 0])
    return np.stack([key % int(graph.n_ent), key // int(graph.n_ent)], 1)


def check_xrules(graph, head, body, lag_lo, lag_hi, row_day, win_lo, win_hi, anchors=None, loop_window=XRULE_LOOP_WINDOW,
                 who="xrule_ground"):
    """The host validation of xrule_ground: (head int32 [R], body, lag_lo, lag_hi int32 [R, L], row_day int32 [n_data], win_lo, win_hi
    int32 [n_day], anchors int64 [S, 2] = (entity, day) sorted by (day, entity)) as contiguous numpy arrays, or ValueError.  ``graph``
    needs n_ent, n_rela_rows and n_time = n_data + 1 (and its rows where ``anchors`` is None); no device is touched."""
    n_ent, n_rows, n_time = int(graph.n_ent), int(graph.n_rela_rows), int(getattr(graph, "n_time", 0) or 0)
    h, b = _int_array(head, "head", who), _int_array(body, "body", who)
    lo, hi = _int_array(lag_lo, "lag_lo", who), _int_array(lag_hi, "lag_hi", who)
    day, w_lo, w_hi = _int_array(row_day, "row_day", who), _int_array(win_lo, "win_lo", who), _int_array(win_hi, "win_hi", who)
    _check_rule_shapes(who, h, b, lag_lo=lo, lag_hi=hi)
    if day.ndim != 1 or n_time != day.shape[0] + 1:
        raise ValueError("%s: not the extrapolation layout: row_day must be [n_data] and the graph's n_time n_data + 1 (got %s and "
                         "n_time=%d)" % (who, day.shape, n_time))
    if w_lo.ndim != 1 or w_lo.shape != w_hi.shape or w_lo.shape[0] < 1:
        raise ValueError("%s: win_lo and win_hi must be [n_day], n_day >= 1 (got %s and %s)" % (who, w_lo.shape, w_hi.shape))
    n_day = w_lo.shape[0]
    if isinstance(loop_window, (bool, np.bool_)) or not isinstance(loop_window, (int, np.integer)) or not 0 <= loop_window < 2 ** 31:
        raise ValueError("%s: loop_window must be a non-negative integer (got %r)" % (who, loop_window))
    _check_rel_range(who, h, b, n_rows - 1)
    if lo.size and (lo.min() < 0 or hi.max() > XRULE_ANY_HI or (lo >= hi).any()):
        raise ValueError("%s: lag range out of order: need 0 <= lag_lo < lag_hi <= %d for every step (got lag_lo %d..%d, lag_hi %d..%d)"
                         % (who, XRULE_ANY_HI, lo.min(), lo.max(), hi.min(), hi.max()))
    if day.size and (day.min() < 0 or day.max() >= n_day):
        raise ValueError("%s: row_day out of range 0..%d (got %d..%d)" % (who, n_day - 1, day.min(), day.max()))
    a = xrule_default_anchors(graph, day) if anchors is None else _check_anchors(who, anchors, n_ent, n_day, "day")
    if w_lo.size and (min(w_lo.min(), w_hi.min()) < 0 or max(w_lo.max(), w_hi.max()) > day.shape[0]):
        raise ValueError("%s: window bound out of range 0..%d (got %d..%d)"
                         % (who, day.shape[0], min(w_lo.min(), w_hi.min()), max(w_lo.max(), w_hi.max())))
    return _as32(h), _as32(b), _as32(lo), _as32(hi), _as32(day), _as32(w_lo), _as32(w_hi), a


def xrule_ground(graph, head, body, lag_lo, lag_hi, row_day, win_lo, win_hi, anchors=None, loop_window=XRULE_LOOP_WINDOW,
                 scratch_bytes=RULE_SCRATCH_BYTES):
    """The four counts of every extrapolation rule (head[i], (body[i], [lag_lo[i], lag_hi[i]))) on the one-graph layout ``graph`` of
    extrapolation.T_RED_GNN (rg_xrule_ground; include/redgnn.h has the definition): int64 [R, 4] on the device = (body_pairs, hits,
    pca_body_pairs, head_pairs) over the pairs ((x, t), y) with (x, t) in ``anchors``, int [S, 2] = (entity, query day), distinct;
    None: xrule_default_anchors.  ``row_day`` [n_data] is the day of every data row, ``win_lo`` / ``win_hi`` [n_day] the forward's row
    window of every query day, ``loop_window`` the lag a full window gives a self-loop.  A step admits a fact of its relation whose lag
    against the query day lies in [lag_lo, lag_hi) and whose row lies in the day's window; [0, 2^31 - 1) is any lag.  Everything is
    validated on the host (ValueError).  The anchors are sorted by (day, entity) and the work is cut into chunks of (rules x blocks of
    consecutive anchors, a multiple of 32) whose bitmaps fit ``scratch_bytes``, as rule_chunking says; each block gets anchor_ptr =
    clip(ptr - s0, 0, s1 - s0), ptr being the first sorted anchor of every day.  The scratch is allocated once and the counts are
    integers added per chunk, so the result does not depend on the budget."""
    scratch_bytes = _check_scratch_bytes(scratch_bytes, "xrule_ground")
    h, b, lo, hi, day, w_lo, w_hi, a = check_xrules(graph, head, body, lag_lo, lag_hi, row_day, win_lo, win_hi, anchors, loop_window)
    L, n_data, n_day, p = b.shape[1], day.shape[0], w_lo.shape[0], _lib.ptr

    def upload(dev, s_c):
        h_d, b_d, lo_d, hi_d, day_d, wl_d, wh_d, e_d, p_d = (
            torch.from_numpy(_as32(x)).to(dev) for x in (h, b, lo, hi, day, w_lo, w_hi, a[:, 0], _block_anchor_ptr(a[:, 1], n_day, s_c)))
        return lambda r0, r1, k, s0, s1, scratch, counts: _lib.check(_lib.lib().rg_xrule_ground(
            graph.handle, p(h_d[r0:r1]), p(b_d[r0:r1]), p(lo_d[r0:r1]), p(hi_d[r0:r1]), r1 - r0, L, p(day_d), n_data, p(wl_d), p(wh_d),
            n_day, int(loop_window), p(e_d[s0:s1]), p(p_d[k]), s1 - s0, p(scratch), p(counts), _lib.stream_ptr()))
    return _ground_chunks("XRULE_EVENTS", graph, h.shape[0], a.shape[0], scratch_bytes, upload)


RULE_APPLY_ALIGN = 256               # csrc/rule_bits.h: RULE_ALIGN
RULE_APPLY_MAX_WORDS = 1 << 40       # ... RULE_MAX_WORDS (words of one bitmap region)
# tools/probe_rule_apply.py sets this to a list to collect (start, after seed + hops, end events, n_rules, n_words) per call of rule_apply
RULE_APPLY_EVENTS = None


def rule_apply_scratch_bytes(n_words):
    """Bytes of the two bitmap regions of ``n_words`` words each (rg_rule_apply_scratch_bytes, restated so that the chunking is a pure
    function; tests hold the two equal): 0 where n_words is outside 1..2^40."""
    n_words = int(n_words)
    if n_words < 1 or n_words > RULE_APPLY_MAX_WORDS:
        return 0
    return 2 * ((4 * n_words + RULE_APPLY_ALIGN - 1) // RULE_APPLY_ALIGN * RULE_APPLY_ALIGN)


def rule_apply_chunking(words, scratch_bytes):
    """The calls of rule_apply: consecutive rule ranges [(r0, r1), ...] covering 0..R in order, given ``words[i]`` = the words of rule
    i's slab (n_ent * ceil(queries of its head relation / 32)).  Greedy: a range takes rules while its slabs' scratch fits
    ``scratch_bytes`` and it has fewer than RULE_MAX_RULES rules; a rule that does not fit alone is a range of its own."""
    words = [int(w) for w in words]
    out, lo, R = [], 0, len(words)
    while lo < R:
        hi, total = lo + 1, words[lo]
        while hi < R and hi - lo < RULE_MAX_RULES and rule_apply_scratch_bytes(max(total + words[hi], 1)) <= scratch_bytes \
                and total + words[hi] <= RULE_APPLY_MAX_WORDS:
            total += words[hi]
            hi += 1
        out.append((lo, hi))
        lo = hi
    return out


def check_rule_apply(n_ent, n_rel, head, body, weight, subs, rels):
    """The host validation of rule_apply: (head int32 [R], body int32 [R, L], weight fp32 [R], subs int32 [B], rels int32 [B]) as
    contiguous numpy arrays, or ValueError."""
    who = "rule_apply"
    h, b, _ = check_rules(n_ent, n_rel, head, body, np.zeros(0, np.int32), who=who)
    w = _check_heads_and_weights(who, h, weight)
    s, r = _int_array(subs, "subs", who), _int_array(rels, "rels", who)
    if s.ndim != 1 or r.ndim != 1 or s.shape[0] != r.shape[0]:
        raise ValueError("%s: need one relation per subject (got subs %s, rels %s)" % (who, s.shape, r.shape))
    n_ent, n_rel = int(n_ent), int(n_rel)
    if s.size and (s.min() < 0 or s.max() >= n_ent):
        raise ValueError("%s: subject id out of range 0..%d (got %d..%d)" % (who, n_ent - 1, s.min(), s.max()))
    if r.size and (r.min() < 0 or r.max() > 2 * n_rel):
        raise ValueError("%s: query relation id out of range 0..%d (2*n_rel; got %d..%d)" % (who, 2 * n_rel, r.min(), r.max()))
    return h, b, w, _as32(s), _as32(r)


def rule_apply(graph, head, body, weight, subs, rels, scratch_bytes=RULE_SCRATCH_BYTES):
    """The rules (head[i], body[i], weight[i]) applied to the queries (subs[b], rels[b], ?) on ``graph`` (rg_rule_apply): four device
    tensors [B, n_ent], ``best`` fp32 (the largest weight among the rules that connect the subject to the entity, 0 where none does),
    ``surv`` fp32 (the product of their 1 - weight, in rule order), ``best_rule`` int32 (the first rule of that weight, -1) and
    ``fired`` int32 (how many do).  ``head`` non-decreasing, weights in (0, 1], relation ids the graph's (0..2*n_rel), duplicate queries
    allowed; all validated on the host (ValueError).  The rules are cut into consecutive ranges whose bitmaps fit ``scratch_bytes``
    (rule_apply_chunking; one rule at least per call); the calls run in rule order on the current stream and carry the four tensors, so
    no bit of the result depends on the budget.  Memory: 16 bytes per (query, entity) cell plus the scratch."""
    if getattr(graph, "n_time", 0):
        raise ValueError("rule_apply: temporal graph: rules are grounded on static and inductive graphs only "
                         "(temporal rules, whose steps carry a direction, are applied by trule_apply)")
    scratch_bytes = _check_scratch_bytes(scratch_bytes, "rule_apply")
    h, b, w, s, r = check_rule_apply(graph.n_ent, graph.n_rel, head, body, weight, subs, rels)
    order = np.argsort(r, kind="stable")
    q_ptr = np.searchsorted(r[order], np.arange(2 * int(graph.n_rel) + 2)).astype(np.int32)
    words = int(graph.n_ent) * ((np.diff(q_ptr).astype(np.int64)[h] + 31) // 32)     # per rule
    return _apply_chunks("rule_apply", "RULE_APPLY_EVENTS", graph, (h, b), w, s[order], order, q_ptr, words, scratch_bytes,
                         lambda *args: _lib.lib().rg_rule_apply(graph.handle, *args))


def _apply_chunks(who, events, graph, rules, w, q_sub, q_row, q_ptr, words, scratch_bytes, entry):
    """What rule_apply, trule_apply and xrule_apply do once the queries are sorted: the four outputs [B, n_ent], the rules cut into
    consecutive calls as rule_apply_chunking says, every call's slabs, and the calls in rule order.  ``rules``: the per-rule int32
    arrays in the entry point's order, (head, body), (head, body, direction) or (head, body, lag_lo, lag_hi); ``w`` their weights;
    ``q_sub`` [B] the subjects in sorted order, ``q_row`` [B] the caller's row of every sorted position, ``q_ptr`` as the entry point
    takes it; ``words`` [R] the words of every rule's slab; ``entry(*args)``: the entry point after its graph.  ``events`` names the module attribute (RULE_APPLY_EVENTS, ...):
    where a probe has set it to a list a call is split into its two phases and the three events around them, the rules and the words
    of the call are collected."""
    dev = _require_gpu(graph.device)
    R, L, B, n_ent = rules[0].shape[0], rules[1].shape[1], q_sub.shape[0], int(graph.n_ent)
    best = torch.zeros((B, n_ent), dtype=torch.float32, device=dev)
    surv = torch.ones((B, n_ent), dtype=torch.float32, device=dev)
    best_rule = torch.full((B, n_ent), -1, dtype=torch.int32, device=dev)
    fired = torch.zeros((B, n_ent), dtype=torch.int32, device=dev)
    chunks = [(r0, r1) for r0, r1 in rule_apply_chunking(words, scratch_bytes) if words[r0:r1].sum() > 0]
    if R == 0 or B == 0 or not chunks:
        return best, surv, best_rule, fired
    slabs = [np.concatenate([[0], np.cumsum(words[r0:r1])]).astype(np.int64) for r0, r1 in chunks]
    need = [rule_apply_scratch_bytes(sl[-1]) for sl in slabs]
    if min(need) == 0:
        raise ValueError("%s: a rule's bitmap of %d words is beyond the bitmaps' range (fewer queries per call)" % (who, max(words)))
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rules_d = [to(a) for a in rules]
    w_d, m_d, qs_d, qr_d, qp_d = (to(a) for a in (w, (np.float32(1.0) - w).astype(np.float32), q_sub, q_row.astype(np.int32), q_ptr))
    slab_d = to(np.concatenate(slabs))
    off = np.concatenate([[0], np.cumsum([len(sl) for sl in slabs])])
    p = _lib.ptr
    with torch.cuda.device(dev):
        scratch = torch.empty(max(need), dtype=torch.uint8, device=dev)
        for c, (r0, r1) in enumerate(chunks):
            def call(phases):
                _lib.check(entry(*(p(a[r0:r1]) for a in rules_d), p(w_d[r0:r1]), p(m_d[r0:r1]), r1 - r0, L, r0, p(qs_d), p(qr_d), p(qp_d),
                                 B, p(slab_d[off[c]:off[c + 1]]), int(slabs[c][-1]), p(scratch), phases, p(best), p(surv), p(best_rule),
                                 p(fired), _lib.stream_ptr()))
            log = globals()[events]                      # read at call time: a test or probe assigns the attribute
            if log is None:
                call(3)
            else:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                call(1)
                ev[1].record()
                call(2)
                ev[2].record()
                log.append((ev[0], ev[1], ev[2], r1 - r0, int(slabs[c][-1])))
    return best, surv, best_rule, fired


# tools/probe_trule_apply.py sets this to a list to collect (start, after seed + hops, end events, n_rules, n_words) per call of trule_apply
TRULE_APPLY_EVENTS = None


def check_trule_apply(graph, head, body, direction, weight, subs, rels, times):
    """The host validation of trule_apply: (head int32 [R], body int32 [R, L], direction int32 [R, L], weight fp32 [R], subs int32 [B],
    rels int32 [B], times int32 [B]) as contiguous numpy arrays, or ValueError.  ``graph`` needs n_ent, n_rela_rows and n_time; no device
    is touched."""
    who = "trule_apply"
    if not int(getattr(graph, "n_time", 0) or 0):
        raise ValueError("%s: static graph (no time ids): static rules are applied by rule_apply" % who)
    h, b, d, _ = check_trules(graph, head, body, direction, np.zeros((0, 2), np.int64), who=who)
    w = _check_heads_and_weights(who, h, weight)
    s, r, t = _int_array(subs, "subs", who), _int_array(rels, "rels", who), _int_array(times, "times", who)
    if s.ndim != 1 or r.shape != s.shape or t.shape != s.shape:
        raise ValueError("%s: need one relation and one time per subject (got subs %s, rels %s, times %s)" % (who, s.shape, r.shape, t.shape))
    n_ent, n_rows, n_time = int(graph.n_ent), int(graph.n_rela_rows), int(graph.n_time)
    if s.size and (s.min() < 0 or s.max() >= n_ent):
        raise ValueError("%s: subject id out of range 0..%d (got %d..%d)" % (who, n_ent - 1, s.min(), s.max()))
    if r.size and (r.min() < 0 or r.max() >= n_rows):
        raise ValueError("%s: query relation id out of range 0..%d (got %d..%d)" % (who, n_rows - 1, r.min(), r.max()))
    if t.size and (t.min() < 0 or t.max() >= n_time):
        raise ValueError("%s: query time id out of range 0..%d (got %d..%d)" % (who, n_time - 1, t.min(), t.max()))
    return h, b, d, w, _as32(s), _as32(r), _as32(t)


def trule_apply(graph, head, body, direction, weight, subs, rels, times, scratch_bytes=RULE_SCRATCH_BYTES):
    """The temporal rules (head[i], (body[i], direction[i]), weight[i]) applied to the queries (subs[b], rels[b], ?, times[b]) on the
    quadruple graph ``graph`` (rg_trule_apply; include/redgnn.h has the definition): the four device tensors [B, n_ent] of rule_apply -
    ``best`` fp32, ``surv`` fp32, ``best_rule`` int32 and ``fired`` int32 - over the rules whose head is the query relation and whose
    steps lead from the subject to the entity through rows whose time stands to the query's as each step's direction says (0 past,
    1 now, 2 future, 3 any).  ``head`` non-decreasing, weights in (0, 1], relation ids the graph's (0..n_rela_rows-1), duplicate
    queries allowed; all validated on the host (ValueError).  The queries are sorted stably by (relation, time id), q_ptr holds the
    first sorted position of every (relation, time id), and the rules are cut into consecutive ranges whose bitmaps fit
    ``scratch_bytes`` (rule_apply_chunking; one rule at least per call); the calls run in rule order on the current stream and carry
    the four tensors, so no bit of the result depends on the budget.  Memory: 16 bytes per (query, entity) cell plus the scratch."""
    scratch_bytes = _check_scratch_bytes(scratch_bytes, "trule_apply")
    h, b, d, w, s, r, t = check_trule_apply(graph, head, body, direction, weight, subs, rels, times)
    n_rows, n_time = int(graph.n_rela_rows), int(graph.n_time)
    key = r.astype(np.int64) * n_time + t
    order = np.argsort(key, kind="stable")
    q_ptr = np.searchsorted(key[order], np.arange(n_rows * n_time + 1)).astype(np.int32)
    per_rel = np.diff(q_ptr[::n_time].astype(np.int64))                            # queries per relation
    words = int(graph.n_ent) * ((per_rel[h] + 31) // 32)                           # per rule
    return _apply_chunks("trule_apply", "TRULE_APPLY_EVENTS", graph, (h, b, d), w, s[order], order, q_ptr, words, scratch_bytes,
                         lambda *args: _lib.lib().rg_trule_apply(graph.handle, *args))


# tools/probe_xrule_apply.py sets this to a list to collect (start, after seed + hops, end events, n_rules, n_words) per call of xrule_apply
XRULE_APPLY_EVENTS = None


def check_xrule_apply(graph, head, body, lag_lo, lag_hi, weight, subs, rels, days, row_day, win_lo, win_hi,
                      loop_window=XRULE_LOOP_WINDOW):
    """The host validation of xrule_apply: (head int32 [R], body, lag_lo, lag_hi int32 [R, L], weight fp32 [R], subs, rels, days int32
    [B], row_day int32 [n_data], win_lo, win_hi int32 [n_day]) as contiguous numpy arrays, or ValueError.  ``graph`` needs n_ent,
    n_rela_rows and n_time = n_data + 1; no device is touched."""
    who = "xrule_apply"
    h, b, lo, hi, day, w_lo, w_hi, _ = check_xrules(graph, head, body, lag_lo, lag_hi, row_day, win_lo, win_hi, np.zeros((0, 2), np.int64),
                                                    loop_window, who=who)
    w = _check_heads_and_weights(who, h, weight)
    s, r, t = _int_array(subs, "subs", who), _int_array(rels, "rels", who), _int_array(days, "days", who)
    if s.ndim != 1 or r.shape != s.shape or t.shape != s.shape:
        raise ValueError("%s: need one relation and one day per subject (got subs %s, rels %s, days %s)" % (who, s.shape, r.shape, t.shape))
    n_ent, n_rows, n_day = int(graph.n_ent), int(graph.n_rela_rows), w_lo.shape[0]
    if s.size and (s.min() < 0 or s.max() >= n_ent):
        raise ValueError("%s: subject id out of range 0..%d (got %d..%d)" % (who, n_ent - 1, s.min(), s.max()))
    if r.size and (r.min() < 0 or r.max() >= n_rows):
        raise ValueError("%s: query relation id out of range 0..%d (got %d..%d)" % (who, n_rows - 1, r.min(), r.max()))
    if t.size and (t.min() < 0 or t.max() >= n_day):
        raise ValueError("%s: query day out of range 0..%d (got %d..%d)" % (who, n_day - 1, t.min(), t.max()))
    return h, b, lo, hi, w, _as32(s), _as32(r), _as32(t), day, w_lo, w_hi


def xrule_query_layout(rels, days, n_rows, n_day):
    """The query layout of rg_xrule_apply for the queries (rels[b], days[b]), relations 0..n_rows-1 and days 0..n_day-1: (order, q_ptr,
    day_ptr, day_of, day_pos).  ``order`` [B] sorts the queries stably by (relation, day); q_ptr int32 [n_rows + 1] holds the first
    sorted position of every relation; the entries are the distinct (relation, day) pairs in sorted order: day_ptr int32 [n_rows + 1]
    the entries of every relation, day_of int32 [D] their days, day_pos int32 [D + 1] their first sorted positions, day_pos[D] = B."""
    r, t = np.asarray(rels, np.int64).reshape(-1), np.asarray(days, np.int64).reshape(-1)
    key = r * int(n_day) + t
    order = np.argsort(key, kind="stable")
    entries, first = np.unique(key[order], return_index=True)
    q_ptr = np.searchsorted(r[order], np.arange(n_rows + 1)).astype(np.int32)
    day_ptr = np.searchsorted(entries // int(n_day), np.arange(n_rows + 1)).astype(np.int32)
    day_pos = np.concatenate([first, [len(r)]]).astype(np.int32)
    return order, q_ptr, day_ptr, (entries % int(n_day)).astype(np.int32), day_pos


def xrule_apply(graph, head, body, lag_lo, lag_hi, weight, subs, rels, days, row_day, win_lo, win_hi, loop_window=XRULE_LOOP_WINDOW,
                scratch_bytes=RULE_SCRATCH_BYTES):
    """The extrapolation rules (head[i], (body[i], [lag_lo[i], lag_hi[i])), weight[i]) applied to the queries (subs[b], rels[b], ?,
    days[b]) on the one-graph layout ``graph`` of extrapolation.T_RED_GNN (rg_xrule_apply; include/redgnn.h has the definition): the
    four device tensors [B, n_ent] of rule_apply - ``best`` fp32, ``surv`` fp32, ``best_rule`` int32 and ``fired`` int32 - over the
    rules whose head is the query relation and whose steps lead from the subject to the entity through rows that each step admits for
    the query day, exactly as xrule_ground admits them for an anchor of that day (``row_day``, ``win_lo`` / ``win_hi`` and
    ``loop_window`` as there).  ``head`` non-decreasing, weights in (0, 1], relation ids the graph's (0..n_rela_rows-1), days in
    0..n_day-1, duplicate queries allowed; all validated on the host (ValueError).  The queries are sorted stably by (relation, day)
    and the distinct days of every relation are listed (xrule_query_layout); the rules are cut into consecutive ranges whose bitmaps
    fit ``scratch_bytes`` (rule_apply_chunking; one rule at least per call); the calls run in rule order on the current stream and
    carry the four tensors, so no bit of the result depends on the budget.  Memory: 16 bytes per (query, entity) cell plus the
    scratch."""
    scratch_bytes = _check_scratch_bytes(scratch_bytes, "xrule_apply")
    h, b, lo, hi, w, s, r, t, day, w_lo, w_hi = check_xrule_apply(graph, head, body, lag_lo, lag_hi, weight, subs, rels, days, row_day,
                                                                  win_lo, win_hi, loop_window)
    n_data, n_day, p = day.shape[0], w_lo.shape[0], _lib.ptr
    order, q_ptr, day_ptr, day_of, day_pos = xrule_query_layout(r, t, int(graph.n_rela_rows), n_day)
    words = int(graph.n_ent) * ((np.diff(q_ptr).astype(np.int64)[h] + 31) // 32)     # per rule
    bound = []                       # the device arrays beyond _apply_chunks' own, uploaded by the first call

    def entry(*a):                   # a: head, body, lag_lo, lag_hi, weight, miss, n_rules, L, rule_base | q_sub, q_row, q_ptr | the rest
        if not bound:
            dev = _require_gpu(graph.device)
            bound.extend(torch.from_numpy(x).to(dev) for x in (day, w_lo, w_hi, day_ptr, day_of, day_pos))
        day_d, wl_d, wh_d, dp_d, do_d, ds_d = bound
        return _lib.lib().rg_xrule_apply(graph.handle, *a[:9], p(day_d), n_data, p(wl_d), p(wh_d), n_day, int(loop_window), *a[9:12],
                                         p(dp_d), p(do_d), p(ds_d), day_of.shape[0], *a[12:])
    return _apply_chunks("xrule_apply", "XRULE_APPLY_EVENTS", graph, (h, b, lo, hi), w, s[order], order, q_ptr, words, scratch_bytes, entry)


def layer_fwd_wp_tickets(frontier, graph, level, walk):
    """(items per queue ticket, work items) rg_layer_fwd would give the word-parallel walk ``walk`` on this hop now (rg_layer_fwd_wp_tickets)."""
    n_items = C.c_int64()
    return int(_lib.lib().rg_layer_fwd_wp_tickets(frontier.handle, graph.handle, level, walk, C.byref(n_items))), int(n_items.value)
