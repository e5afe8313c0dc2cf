"""ctypes binding of libredgnn.so — the C-ABI declared in include/redgnn.h.

This is the binding a maintainer of the reference would add.  There is no
CPU fallback: if the HIP library is missing, loading fails loudly.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RG_LIB") or os.path.join(_PKG, "libredgnn.so")      # RG_LIB: an alternative build (kernel A/B runs)

# every symbol include/redgnn.h declares (tests check the library exports all of them)
SYMBOLS = [
    "rg_last_error", "rg_version", "rg_hipgraph_fill_nodes",
    "rg_graph_create", "rg_graph_create_device", "rg_graph_export_packs", "rg_tgraph_create", "rg_tgraph_create_excluding", "rg_graph_destroy", "rg_graph_n_fact", "rg_graph_export", "rg_graph_export_out_by_tail",
    "rg_frontier_workspace_bytes", "rg_frontier_create", "rg_frontier_destroy", "rg_frontier_reset",
    "rg_frontier_reset_nodes", "rg_frontier_expand", "rg_frontier_nodes", "rg_frontier_edges_scratch_bytes", "rg_frontier_edges",
    "rg_layer_fwd_scratch_bytes", "rg_layer_fwd", "rg_layer_fwd_plan", "rg_layer_fwd_wp_tickets", "rg_layer_fwd_single_source", "rg_tlayer_fwd", "rg_xlayer_fwd", "rg_frontier_set_window", "rg_layer_bwd_scratch_bytes", "rg_layer_bwd", "rg_tlayer_bwd_scratch_bytes", "rg_tlayer_bwd", "rg_xlayer_bwd", "rg_dense_fwd_supported", "rg_dense_scratch_bytes", "rg_dense_fwd", "rg_dense_fwd_dev", "rg_dense_train_fwd", "rg_dense_train_fwd_as", "rg_rows_addmm", "rg_dense_train_bwd", "rg_dense_train_bwd2", "rg_split3_roundtrip", "rg_split3_product_check", "rg_gram_tn_scratch_bytes", "rg_gram_tn", "rg_rank",
    "rg_frontier_expand_async", "rg_frontier_expand_nodes_async", "rg_frontier_set_edge_hint", "rg_frontier_count_ptr", "rg_frontier_level_counts", "rg_attn_tables",
    "rg_explain_scratch_bytes", "rg_explain_seed", "rg_explain_count", "rg_explain_emit", "rg_explain_gather",
    "rg_topk",
    "rg_attn_profile",
    "rg_graph_export_time", "rg_graph_export_array", "rg_texplain_count", "rg_texplain_emit", "rg_tattn_profile",
    "rg_segment_rank", "rg_segment_topk",
    "rg_xexplain_count", "rg_xexplain_emit",
    "rg_xattn_profile", "rg_rows_linear",
    "rg_segment_eval",
    "rg_paths_scratch_bytes", "rg_paths_topk",
    "rg_digraph_layer_fwd_scratch_bytes", "rg_digraph_layer_fwd", "rg_digraph_tlayer_fwd",
    "rg_digraph_layer_bwd_scratch_bytes", "rg_digraph_layer_bwd", "rg_digraph_tlayer_bwd",
    "rg_digraph_layer_fwd_gated_scratch_bytes", "rg_digraph_layer_fwd_gated",
    "rg_digraph_layer_bwd_gated_scratch_bytes", "rg_digraph_layer_bwd_gated",
    "rg_digraph_layer_fwd_gates", "rg_digraph_layer_bwd_gates", "rg_mask_step",
    "rg_mask_tie_grad_scratch_bytes", "rg_mask_tie_grad", "rg_mask_tie_gates",
    "rg_digraph_hop_ranges", "rg_digraph_hop_index_scratch_bytes", "rg_digraph_hop_index",
    "rg_rule_ground_scratch_bytes", "rg_rule_ground",
    "rg_rule_apply_scratch_bytes", "rg_rule_apply",
    "rg_trule_ground_scratch_bytes", "rg_trule_ground",
    "rg_trule_apply",
    "rg_xrule_ground",
    "rg_xrule_apply",
]

_lib = None


class NativeError(RuntimeError):
    pass


def lib():
    """The loaded library; raises if it has not been built (``python -m red_gnn_amd.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "libredgnn.so is missing at %s: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback." % LIB_PATH)
    # torch bundles its own HIP runtime (libamdhip64.so.7); it must be loaded first so that this
    # library binds to the SAME runtime (one device context, shared streams and allocations).
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    L.rg_last_error.restype = C.c_char_p
    L.rg_version.restype = C.c_int
    L.rg_hipgraph_fill_nodes.argtypes = [vp]
    L.rg_graph_create.argtypes = [i32, i32, vp, i64, C.c_int, C.POINTER(vp)]
    L.rg_graph_create_device.argtypes = [i32, i32, vp, i64, C.c_int, vp, C.POINTER(vp)]
    L.rg_graph_export_packs.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), vp, vp, vp, vp]
    L.rg_tgraph_create.argtypes = [i32, i32, i32, vp, i64, C.POINTER(vp)]
    L.rg_tgraph_create_excluding.argtypes = [i32, i32, i32, vp, i64, vp, i64, C.POINTER(vp)]
    L.rg_graph_destroy.argtypes = [vp]
    L.rg_graph_n_fact.argtypes = [vp]
    L.rg_graph_n_fact.restype = i64
    L.rg_graph_export.argtypes = [vp, vp, vp, vp, vp]
    L.rg_graph_export_out_by_tail.argtypes = [vp, vp, vp, vp]
    L.rg_frontier_workspace_bytes.argtypes = [i32, i32, i32]
    L.rg_frontier_workspace_bytes.restype = sz
    L.rg_frontier_create.argtypes = [i32, i32, i32, vp, sz, C.POINTER(vp)]
    L.rg_frontier_destroy.argtypes = [vp]
    L.rg_frontier_reset.argtypes = [vp, vp, vp]
    L.rg_frontier_reset_nodes.argtypes = [vp, vp, i64, vp]
    L.rg_frontier_expand.argtypes = [vp, vp, C.POINTER(i64), vp]
    L.rg_frontier_expand_async.argtypes = [vp, vp, vp]
    L.rg_frontier_expand_nodes_async.argtypes = [vp, vp, vp, vp, vp]
    L.rg_frontier_set_edge_hint.argtypes = [vp, i64]
    L.rg_attn_tables.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rg_frontier_count_ptr.argtypes = [vp]
    L.rg_frontier_count_ptr.restype = vp
    L.rg_frontier_level_counts.argtypes = [vp, C.POINTER(i64), vp]
    L.rg_frontier_nodes.argtypes = [vp, vp, vp, vp, vp]
    L.rg_frontier_edges_scratch_bytes.argtypes = [i64]
    L.rg_frontier_edges_scratch_bytes.restype = sz
    L.rg_frontier_edges.argtypes = [vp, vp, i32, vp, i64, vp, vp, vp, vp]
    L.rg_layer_fwd_scratch_bytes.argtypes = [vp, vp, i32]
    L.rg_layer_fwd_scratch_bytes.restype = sz
    L.rg_layer_fwd.argtypes = [vp, vp, i32, i64, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, sz, i32, vp]
    L.rg_layer_fwd_plan.argtypes = [vp, vp, i32, i64, i64, i64, i32]
    L.rg_layer_fwd_wp_tickets.argtypes = [vp, vp, i32, i32, C.POINTER(i64)]
    L.rg_layer_fwd_single_source.argtypes = [vp, vp, i32]
    L.rg_tlayer_fwd.argtypes = [vp, vp, i32, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, sz, vp]
    L.rg_xlayer_fwd.argtypes = [vp, vp, i32, i64, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, sz, vp]
    L.rg_frontier_set_window.argtypes = [vp, vp, vp, i32]
    L.rg_layer_bwd_scratch_bytes.argtypes = [vp, vp, i32, i32]
    L.rg_layer_bwd_scratch_bytes.restype = sz
    L.rg_layer_bwd.argtypes = [vp, vp, i32, i64, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32,
                               vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.rg_tlayer_bwd_scratch_bytes.argtypes = [vp, vp, i32, i32]
    L.rg_tlayer_bwd_scratch_bytes.restype = sz
    L.rg_tlayer_bwd.argtypes = [vp, vp, i32, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32,
                                vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.rg_xlayer_bwd.argtypes = [vp, vp, i32, i64, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, i32,
                                vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.rg_dense_fwd_supported.argtypes = [i32, i32]
    L.rg_dense_fwd.argtypes = [i64, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, i64, vp]
    L.rg_dense_scratch_bytes.argtypes = [i32, i32]
    L.rg_dense_scratch_bytes.restype = i64
    L.rg_dense_fwd_dev.argtypes = [i64, vp, i64, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, i64, vp]
    L.rg_dense_train_fwd.argtypes = [i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rg_dense_train_fwd_as.argtypes = [i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.rg_rows_addmm.argtypes = [vp, i64, vp, i64, i32, vp, i32, i64, vp, i64, vp]
    L.rg_dense_train_bwd.argtypes = [i64, i32, vp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rg_dense_train_bwd2.argtypes = [i64, i32, vp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rg_rank.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.rg_topk.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.rg_split3_roundtrip.argtypes = [vp, i64, i32, vp, vp, vp]
    L.rg_gram_tn_scratch_bytes.argtypes = [i32, i32]
    L.rg_gram_tn_scratch_bytes.restype = sz
    L.rg_gram_tn.argtypes = [vp, i64, i32, vp, i64, i32, i64, vp, vp, vp, sz, vp]
    L.rg_split3_product_check.argtypes = [i32, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.rg_explain_scratch_bytes.argtypes = [vp]
    L.rg_explain_scratch_bytes.restype = sz
    L.rg_explain_seed.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.rg_explain_count.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp, vp, vp, sz,
                                   C.POINTER(i64), vp]
    L.rg_explain_emit.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp, vp, vp, vp]
    L.rg_explain_gather.argtypes = [i64, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.rg_attn_profile.argtypes = [vp, vp, i32, i32, i32, i64, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.rg_graph_export_time.argtypes = [vp, vp, vp]
    L.rg_graph_export_array.argtypes = [vp, C.c_char_p, vp, vp, vp]
    L.rg_texplain_count.argtypes = L.rg_explain_count.argtypes
    L.rg_texplain_emit.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp, vp, vp, vp, vp]
    L.rg_tattn_profile.argtypes = [vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.rg_segment_rank.argtypes = [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.rg_segment_topk.argtypes = [vp, vp, i64, vp, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.rg_segment_eval.argtypes = [vp, vp, i64, vp, i32, vp, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.rg_xexplain_count.argtypes = L.rg_explain_count.argtypes
    L.rg_xexplain_emit.argtypes = L.rg_texplain_emit.argtypes
    L.rg_rows_linear.argtypes = [vp, i64, i64, i32, vp, vp, i32, vp, i64, vp]
    L.rg_xattn_profile.argtypes = [vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.rg_paths_scratch_bytes.argtypes = [i64, i32]
    L.rg_paths_scratch_bytes.restype = sz
    L.rg_paths_topk.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.rg_digraph_layer_fwd_scratch_bytes.argtypes = [vp, i32, i32]
    L.rg_digraph_layer_fwd_scratch_bytes.restype = sz
    L.rg_digraph_layer_fwd.argtypes = [i32, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp,
                                       vp, sz, vp]
    L.rg_digraph_tlayer_fwd.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32,
                                        vp, vp, i32, vp, vp, vp, sz, vp]
    L.rg_digraph_layer_bwd_scratch_bytes.argtypes = [vp, i32, i32, i32]
    L.rg_digraph_layer_bwd_scratch_bytes.restype = sz
    L.rg_digraph_layer_bwd.argtypes = [i32, i32, i64, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp,
                                       vp, vp, vp, sz, vp]
    L.rg_digraph_tlayer_bwd.argtypes = [i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp,
                                        i32, vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]
    # the gated, replicated forms: (n_rep, t, gate_lo, gate_hi) in front of the ungated arguments
    L.rg_digraph_layer_fwd_gated_scratch_bytes.argtypes = [vp, i32, i32, i32]
    L.rg_digraph_layer_fwd_gated_scratch_bytes.restype = sz
    L.rg_digraph_layer_fwd_gated.argtypes = [i32, vp, vp, vp] + L.rg_digraph_layer_fwd.argtypes
    L.rg_digraph_layer_bwd_gated_scratch_bytes.argtypes = [vp, i32, i32, i32, i32]
    L.rg_digraph_layer_bwd_gated_scratch_bytes.restype = sz
    L.rg_digraph_layer_bwd_gated.argtypes = [i32, vp, vp, vp] + L.rg_digraph_layer_bwd.argtypes
    # a gate per (replica, edge): (n_rep, gate) in front of the ungated arguments; the _gated scratch functions serve them
    L.rg_digraph_layer_fwd_gates.argtypes = [i32, vp] + L.rg_digraph_layer_fwd.argtypes
    L.rg_digraph_layer_bwd_gates.argtypes = [i32, vp] + L.rg_digraph_layer_bwd.argtypes
    f32 = C.c_float
    L.rg_mask_step.argtypes = [i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rg_mask_tie_grad_scratch_bytes.argtypes = [vp, i32, i32]
    L.rg_mask_tie_grad_scratch_bytes.restype = sz
    L.rg_mask_tie_grad.argtypes = [i32, i64, i32, i64, vp, vp, vp, vp, vp, vp, sz, vp]
    L.rg_mask_tie_gates.argtypes = [i32, i64, i32, vp, vp, vp, vp]
    L.rg_digraph_hop_ranges.argtypes =[vp, vp, i64, i32, i32, vp, vp, vp, vp, C.POINTER(i32), vp]
    L.rg_digraph_hop_index_scratch_bytes.argtypes = [i64]
    L.rg_digraph_hop_index_scratch_bytes.restype = sz
    L.rg_digraph_hop_index.argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, vp, i64, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                       vp, sz, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), vp]
    L.rg_rule_ground_scratch_bytes.argtypes = [i32, i32, i32]
    L.rg_rule_ground_scratch_bytes.restype = sz
    L.rg_rule_ground.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp]
    L.rg_rule_apply_scratch_bytes.argtypes = [i64]
    L.rg_rule_apply_scratch_bytes.restype = sz
    L.rg_rule_apply.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, i64, vp, i32, vp, vp, vp, vp, vp]
    L.rg_trule_ground_scratch_bytes.argtypes = [i32, i32, i32]
    L.rg_trule_ground_scratch_bytes.restype = sz
    L.rg_trule_ground.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp]
    L.rg_xrule_ground.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp]
    L.rg_trule_apply.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, i64, vp, i32, vp, vp, vp, vp, vp]
    L.rg_xrule_apply.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32,
                                 vp, i64, vp, i32, vp, vp, vp, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise NativeError(lib().rg_last_error().decode("utf-8", "replace"))


def ptr(t):
    """Device (or host) pointer of a torch tensor / numpy array; None -> NULL."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
