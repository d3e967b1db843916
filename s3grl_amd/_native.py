"""ctypes binding of libs3grl_hip.so (the C ABI declared in include/s3grl.h).

There is NO fallback: if the shared library is missing or a call fails, this module raises.
Build it with `python -c "import __graft_entry__ as g; g.build()"` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libs3grl_hip.so"

# status codes (include/s3grl.h)
OK = 0
ERR_INVALID_ARGUMENT = 1
ERR_NOT_IMPLEMENTED = 2
ERR_NO_FEATURES = 3
ERR_OUT_OF_MEMORY = 4
ERR_HIP = 5
ERR_NO_DEVICE = 6
ERR_GRAPH_TOO_LARGE = 7
ERR_SELF_LINK = 8

MODE_POS, MODE_POS_PLUS, MODE_SOP, MODE_SOP_RESTRICTED = 0, 1, 2, 3
STRATEGY = {"intersection": 0, "union": 1}

# every symbol include/s3grl.h declares; tests check the library exports all of them
SYMBOLS = [
    "s3grl_abi_version", "s3grl_status_string", "s3grl_last_error",
    "s3grl_context_create", "s3grl_context_preload", "s3grl_context_destroy", "s3grl_context_timings",
    "s3grl_context_set_profiling", "s3grl_context_trim", "s3grl_plan_gather_traffic",
    "s3grl_graph_create", "s3grl_graph_create_directed", "s3grl_graph_destroy",
    "s3grl_plan_create", "s3grl_plan_create_sets", "s3grl_walk_sets", "s3grl_plan_destroy", "s3grl_plan_get_stats", "s3grl_plan_total_rows", "s3grl_plan_counts", "s3grl_plan_row_ptr",
    "s3grl_plan_row_nodes", "s3grl_plan_export_subgraphs", "s3grl_plan_link_cost", "s3grl_run",
    "s3grl_sop_create", "s3grl_sop_create_weighted", "s3grl_sop_destroy", "s3grl_sop_run", "s3grl_sop_features",
    "s3grl_sop_layout", "s3grl_sop_class_links",
    "s3grl_features_create", "s3grl_features_destroy", "s3grl_features_info", "s3grl_run_features",
    "s3grl_centre_pool_forward", "s3grl_centre_pool_backward", "s3grl_calibration_read",
    "s3grl_subgraphs_create", "s3grl_subgraphs_counts", "s3grl_subgraphs_export", "s3grl_subgraphs_destroy",
    "s3grl_gcn_norm", "s3grl_gcn_propagate", "s3grl_sort_pool_forward", "s3grl_sort_pool_backward",
    "s3grl_skipgram_create", "s3grl_skipgram_epoch", "s3grl_skipgram_step_windows", "s3grl_skipgram_export_windows",
    "s3grl_skipgram_state", "s3grl_skipgram_weight", "s3grl_skipgram_destroy",
    "s3grl_mf_layout", "s3grl_mf_create", "s3grl_mf_epoch", "s3grl_mf_step_pairs", "s3grl_mf_export_draws",
    "s3grl_mf_score", "s3grl_mf_state", "s3grl_mf_destroy",
    "s3grl_signnet_layout", "s3grl_signnet_create", "s3grl_signnet_fit_epoch", "s3grl_signnetruns_fit_epoch",
    "s3grl_signnet_draws",
    "s3grl_signnet_step", "s3grl_signnet_score", "s3grl_signnet_read_state", "s3grl_signnet_write_state",
    "s3grl_signnet_destroy",
    "s3grl_linkclf_layout", "s3grl_linkclf_create", "s3grl_linkclf_fit", "s3grl_linkclf_newton_step",
    "s3grl_linkclf_state", "s3grl_linkclf_predict", "s3grl_linkclf_destroy",
    "s3grl_metrics_layout", "s3grl_metrics_create", "s3grl_metrics_ranked", "s3grl_metrics_mrr",
    "s3grl_metrics_destroy",
    "s3grl_heuristics_create", "s3grl_heuristics_pairs", "s3grl_heuristics_ppr", "s3grl_heuristics_katz",
    "s3grl_heuristics_destroy",
    "s3grl_sketch_build", "s3grl_sketch_cardinality", "s3grl_sketch_pairs", "s3grl_masked_sketch_pairs",
    "s3grl_cn_count", "s3grl_cn_fill", "s3grl_segment_sum",
    "s3grl_cn_split_count", "s3grl_cn_split_fill", "s3grl_segment_wsum", "s3grl_segment_dot",
    "s3grl_gae_keys", "s3grl_gae_negatives", "s3grl_gae_incidence", "s3grl_gae_decode", "s3grl_gae_backward",
    "s3grl_nbr_aggregate", "s3grl_segment_mean_forward", "s3grl_segment_mean_backward",
    "s3grl_gic_normalise", "s3grl_gic_cluster_forward", "s3grl_gic_cluster_backward", "s3grl_gic_disc_forward",
    "s3grl_gic_disc_backward",
    "s3grl_wp_layout", "s3grl_wp_attention_forward", "s3grl_wp_attention_backward", "s3grl_wp_walk_forward",
    "s3grl_wp_walk_backward",
    "s3grl_candidates_layout", "s3grl_candidates_count", "s3grl_candidates_fill", "s3grl_segment_topk",
]


class Cfg(C.Structure):
    _fields_ = [("mode", C.c_int32), ("num_hops", C.c_int32), ("sign_k", C.c_int32),
                ("strategy", C.c_int32), ("directed", C.c_int32), ("flags", C.c_uint32),
                ("rw_m", C.c_int32), ("rw_M", C.c_int32), ("seed", C.c_uint32),
                ("max_nodes_per_hop", C.c_int32), ("ratio_per_hop", C.c_double),
                ("reserved", C.c_int32 * 4)]


class NodeSets(C.Structure):
    _fields_ = [("set_ptr", C.c_void_p), ("set_nodes", C.c_void_p), ("num_sets", C.c_int64),
                ("num_set_nodes", C.c_int64), ("per_link", C.c_int32), ("reserved", C.c_int32)]


class SubgraphCfg(C.Structure):
    _fields_ = [("num_hops", C.c_int32), ("seed", C.c_uint32), ("max_nodes_per_hop", C.c_int32),
                ("lds_budget", C.c_int32), ("ratio_per_hop", C.c_double), ("reserved", C.c_int32 * 4)]


class SkipgramCfg(C.Structure):
    _fields_ = [("dim", C.c_int32), ("walk_length", C.c_int32), ("context_size", C.c_int32),
                ("walks_per_node", C.c_int32), ("num_negative_samples", C.c_int32), ("seed", C.c_uint32),
                ("p", C.c_double), ("q", C.c_double), ("reserved", C.c_int32 * 4)]


class MfCfg(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("num_layers", C.c_int32), ("dropout", C.c_double), ("seed", C.c_uint32),
                ("reserved", C.c_int32 * 3)]


class WpBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("node_ptr", "link", "in_ptr", "in_nbr", "in_dst", "in_flag", "out_ptr",
                                          "out_nbr", "out_arc")] + \
               [(n, C.c_int64) for n in ("num_links", "num_nodes", "num_arcs", "max_nodes", "max_arcs")]


# s3grl_wp_*'s envelope (csrc/s3grl_walkpool.hip)
WP_MAX_NODES, WP_MAX_WALK, WP_MAX_HEADS, WP_MAX_HIDDEN = 4096, 16, 64, 4096

# s3grl_mf_*'s envelope (csrc/s3grl_mf.hip)
MF_MAX_HIDDEN, MF_MIN_LAYERS, MF_MAX_LAYERS, MF_MAX_BATCH = 128, 2, 4, 1024


class SignnetCfg(C.Structure):
    _fields_ = [("in_width", C.c_int32), ("hidden", C.c_int32), ("pool_mode", C.c_int32), ("seed", C.c_uint32),
                ("dropout", C.c_double), ("reserved", C.c_int32 * 4)]


# s3grl_signnet_*'s envelope and pool modes (csrc/s3grl_signnet.hip)
SIGNNET_MAX_HIDDEN, SIGNNET_MAX_BATCH, SIGNNET_MAX_WIDTH = 256, 64, 1 << 20
SIGNNET_POOL = {"": 0, "mean": 1, "sum": 2}
SIGNNET_MAX_RUNS = 16    # members of one s3grl_signnetruns_fit_epoch call

# s3grl_linkclf_*'s envelope (csrc/s3grl_linkclf.hip) and what its `done` says
LINKCLF_MAX_DIM = 128
LINKCLF_DONE = {0: "running", 1: "converged", 2: "no step accepted", 3: "Hessian not positive definite"}

# s3grl_label: the node-labelling tricks of reference construct_pyg_graph (utils.py:289-307); any other
# name gives zeros there and here
LABELS = {"drnl": 0, "de": 1, "de+": 2, "hop": 3, "zo": 4, "degree": 5}
LABEL_ZEROS = 6

# s3grl_nbr_aggregate's scale_side
SCALE_NONE, SCALE_OWN, SCALE_NEIGHBOUR = 0, 1, 2

# s3grl_gic_*'s shape limits (S3GRL_GIC_MAX_DIM, S3GRL_GIC_MAX_CLUSTERS)
GIC_MAX_DIM, GIC_MAX_CLUSTERS = 4096, 256

# s3grl_candidates_* / s3grl_segment_topk's envelope (csrc/s3grl_recommend.hip)
CANDIDATES_MAX_HOPS, CANDIDATES_LDS_NODES, TOPK_MAX_K = 8, 524288, 1024

ABI_VERSION = 6
FLAG_FULL_STATS, FLAG_NO_FOLD, FLAG_COUNT_ONLY = 1, 2, 4


class PlanStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "num_links", "total_rows", "total_nodes", "total_volume", "total_sub_edges",
        "total_support", "num_row_pairs", "max_nodes", "workspace_bytes", "folded_links",
        "extracted_nodes", "oriented_entries", "hub_links", "hub_read_bytes", "hub_endpoint_entries", "hub_nodes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class S3GRLError(RuntimeError):
    def __init__(self, status, what, detail):
        self.status = status
        super().__init__(f"{what}: {detail}" if detail else what)


_lib = None


def lib():
    """The loaded library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; import it FIRST so that the dynamic loader binds
    # this library to the same HIP runtime (one runtime per process: device pointers and
    # streams are shared with torch).
    import torch  # noqa: F401

    path = Path(os.environ.get("S3GRL_LIB", LIB_PATH))
    if not path.exists():
        raise ImportError(
            f"{path} not found: the HIP engine is not built. Run __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(str(path))
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    L.s3grl_abi_version.restype = i32
    L.s3grl_status_string.restype = C.c_char_p
    L.s3grl_status_string.argtypes = [i32]
    L.s3grl_last_error.restype = C.c_char_p
    proto = {
        "s3grl_context_create": [i32, vp, C.POINTER(vp)],
        "s3grl_context_preload": [vp, C.c_uint32, C.POINTER(C.c_double)],
        "s3grl_context_destroy": [vp],
        "s3grl_context_timings": [vp, C.POINTER(C.c_double)],
        "s3grl_context_set_profiling": [vp, i32],
        "s3grl_context_trim": [vp, C.POINTER(i64)],
        "s3grl_plan_gather_traffic": [vp, vp, vp, C.POINTER(i64)],
        "s3grl_graph_create": [vp, i64, vp, vp, i64, C.POINTER(vp)],
        "s3grl_graph_create_directed": [vp, i64, vp, vp, vp, vp, i64, C.POINTER(vp)],
        "s3grl_graph_destroy": [vp],
        "s3grl_plan_create": [vp, vp, vp, i64, C.POINTER(Cfg), C.POINTER(vp)],
        "s3grl_plan_create_sets": [vp, vp, vp, i64, C.POINTER(Cfg), C.POINTER(NodeSets), C.POINTER(vp)],
        "s3grl_walk_sets": [vp, vp, vp, i64, i32, i32, C.c_uint32, vp, vp],
        "s3grl_plan_destroy": [vp],
        "s3grl_plan_get_stats": [vp, C.POINTER(PlanStats)],
        "s3grl_plan_total_rows": [vp, C.POINTER(i64)],
        "s3grl_plan_counts": [vp, C.POINTER(i64)],
        "s3grl_plan_row_ptr": [vp, vp],
        "s3grl_plan_row_nodes": [vp, vp],
        "s3grl_plan_export_subgraphs": [vp, vp, vp, vp],
        "s3grl_plan_link_cost": [vp, vp],
        "s3grl_run": [vp, vp, vp, i64, i64, vp],
        "s3grl_sop_create": [vp, vp, vp, i64, i64, i32, C.POINTER(vp)],
        "s3grl_sop_create_weighted": [vp, vp, vp, i64, i64, i32, vp, C.POINTER(vp)],
        "s3grl_sop_destroy": [vp],
        "s3grl_sop_run": [vp, vp, vp, i64, vp],
        "s3grl_sop_features": [vp, vp, vp],
        "s3grl_sop_layout": [i64, i32, C.POINTER(i32)],
        "s3grl_sop_class_links": [vp, C.POINTER(i64)],
        "s3grl_features_create": [vp, vp, i64, i64, i64, i32, C.POINTER(vp)],
        "s3grl_features_destroy": [vp],
        "s3grl_features_info": [vp, C.POINTER(i64), C.POINTER(i32)],
        "s3grl_run_features": [vp, vp, vp, vp],
        "s3grl_centre_pool_forward": [vp, vp, vp, i64, i64, i32, vp],
        "s3grl_centre_pool_backward": [vp, vp, vp, i64, i64, i32, vp, vp],
        "s3grl_calibration_read": [vp, vp, i64, i32, i64, i32, C.POINTER(i64)],
        "s3grl_subgraphs_create": [vp, vp, vp, vp, i64, C.POINTER(SubgraphCfg), i32, C.POINTER(vp)],
        "s3grl_subgraphs_counts": [vp, C.POINTER(i64)],
        "s3grl_subgraphs_export": [vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "s3grl_subgraphs_destroy": [vp],
        "s3grl_gcn_norm": [vp, i64, vp, vp, vp],
        "s3grl_gcn_propagate": [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp],
        "s3grl_sort_pool_forward": [vp, vp, vp, i64, i64, i64, i64, i64, vp, vp, vp],
        "s3grl_sort_pool_backward": [vp, i64, i64, i64, vp, vp, i64, vp],
        "s3grl_skipgram_create": [vp, i64, vp, vp, i64, C.POINTER(SkipgramCfg), vp, C.POINTER(vp)],
        "s3grl_skipgram_epoch": [vp, i64, i64, C.c_float, vp],
        "s3grl_skipgram_step_windows": [vp, vp, i64, vp, i64, C.c_float, vp],
        "s3grl_skipgram_export_windows": [vp, i64, i64, i64, vp, vp],
        "s3grl_skipgram_state": [vp, vp, vp, vp, C.POINTER(i64)],
        "s3grl_skipgram_weight": [vp, C.POINTER(vp)],
        "s3grl_skipgram_destroy": [vp],
        "s3grl_mf_layout": [i32, i32, i64, C.POINTER(i32)],
        "s3grl_mf_create": [vp, i64, C.POINTER(MfCfg), vp, vp, C.POINTER(vp)],
        "s3grl_mf_epoch": [vp, i64, vp, i64, i64, C.c_double, vp],
        "s3grl_mf_step_pairs": [vp, vp, i64, vp, C.c_double, vp],
        "s3grl_mf_export_draws": [vp, i64, i64, i64, i64, vp, vp, vp],
        "s3grl_mf_score": [vp, vp, i64, vp],
        "s3grl_mf_state": [vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)],
        "s3grl_mf_destroy": [vp],
        "s3grl_signnet_layout": [i32, i64, i32, i32, C.POINTER(i32)],
        "s3grl_signnet_create": [vp, C.POINTER(SignnetCfg), C.POINTER(vp)],
        "s3grl_signnet_fit_epoch": [vp, i64, vp, i64, vp, vp, i64, i64, C.c_double, vp],
        "s3grl_signnetruns_fit_epoch": [C.POINTER(vp), i32, i64, vp, i64, vp, vp, i64, i64, C.POINTER(C.c_double), vp],
        "s3grl_signnet_draws": [vp, i64, i64, i64, i64, vp, vp, i64, vp],
        "s3grl_signnet_step": [vp, vp, i64, vp, vp, i64, vp, i64, vp, vp, C.c_double, vp],
        "s3grl_signnet_score": [vp, vp, i64, vp, i64, vp],
        "s3grl_signnet_read_state": [vp, i32, vp, C.POINTER(i64)],
        "s3grl_signnet_write_state": [vp, i32, vp, C.POINTER(i64)],
        "s3grl_signnet_destroy": [vp],
        "s3grl_linkclf_layout": [i32, C.POINTER(i32)],
        "s3grl_linkclf_create": [vp, i32, C.c_double, C.c_double, i32, C.POINTER(vp)],
        "s3grl_linkclf_fit": [vp, vp, i64, vp, vp, i64, vp],
        "s3grl_linkclf_newton_step": [vp, vp, i64, vp, vp, i64],
        "s3grl_linkclf_state": [vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32),
                                C.POINTER(i32)],
        "s3grl_linkclf_predict": [vp, vp, i64, vp, i64, vp, vp, vp, vp],
        "s3grl_linkclf_destroy": [vp],
        "s3grl_metrics_layout": [i64, C.POINTER(i32)],
        "s3grl_metrics_create": [vp, C.POINTER(vp)],
        "s3grl_metrics_ranked": [vp, vp, vp, i64, i64, C.POINTER(i64), i32, C.POINTER(i64), C.POINTER(C.c_double),
                                 C.POINTER(i64)],
        "s3grl_metrics_mrr": [vp, vp, vp, i64, i64, vp, C.POINTER(C.c_double), C.POINTER(i64)],
        "s3grl_metrics_destroy": [vp],
        "s3grl_heuristics_create": [vp, i64, vp, vp, vp, i64, C.POINTER(vp)],
        "s3grl_heuristics_pairs": [vp, C.c_int32, vp, i64, vp],
        "s3grl_heuristics_ppr": [vp, vp, i64, vp, i64, C.c_double, C.c_double, C.c_int32, C.c_int32, vp, vp],
        "s3grl_heuristics_katz": [vp, vp, i64, vp, i64, C.c_double, C.c_int32, C.c_int32, vp],
        "s3grl_heuristics_destroy": [vp],
        "s3grl_sketch_build": [vp, i64, vp, vp, i64, i32, i32, i32, C.c_uint32, vp, vp],
        "s3grl_sketch_cardinality": [vp, i32, vp, C.c_double, vp, i64, vp],
        "s3grl_sketch_pairs": [vp, i64, i32, i32, i32, vp, vp, vp, C.c_double, vp, i64, vp, vp, vp, vp, vp],
        "s3grl_masked_sketch_pairs": [vp, i64, vp, vp, i64, i32, i32, i32, vp, vp, vp, C.c_double, vp, i64, vp, vp, vp,
                                      vp, vp],
        "s3grl_cn_count": [vp, i64, vp, vp, i64, vp, i64, i32, vp],
        "s3grl_cn_fill": [vp, i64, vp, vp, i64, vp, i64, i32, vp, i64, vp],
        "s3grl_segment_sum": [vp, vp, i64, i64, vp, vp, i64, vp],
        "s3grl_cn_split_count": [vp, i64, vp, vp, i64, vp, i64, i32, vp],
        "s3grl_cn_split_fill": [vp, i64, vp, vp, i64, vp, i64, i32, vp, vp, i64, vp, vp],
        "s3grl_segment_wsum": [vp, vp, i64, i64, vp, vp, vp, i64, vp],
        "s3grl_segment_dot": [vp, vp, i64, vp, i64, i64, vp, vp, vp],
        "s3grl_gae_keys": [vp, i64, vp, vp, i64, vp, C.POINTER(i64)],
        "s3grl_gae_negatives": [vp, i64, vp, i64, i64, C.c_uint32, i64, vp, vp, C.POINTER(i64)],
        "s3grl_gae_incidence": [vp, i64, vp, vp, i64, vp, vp],
        "s3grl_gae_decode": [vp, i64, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp],
        "s3grl_gae_backward": [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "s3grl_nbr_aggregate": [vp, i64, i64, vp, vp, vp, vp, vp, i32, C.c_float, vp, vp],
        "s3grl_segment_mean_forward": [vp, vp, vp, i64, i64, i64, vp, vp],
        "s3grl_segment_mean_backward": [vp, vp, i64, i64, i64, vp, vp],
        "s3grl_gic_normalise": [vp, i64, i64, vp, i64, vp, vp],
        "s3grl_gic_cluster_forward": [vp, i64, i64, i64, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "s3grl_gic_cluster_backward": [vp, i64, i64, i64, C.c_float, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "s3grl_gic_disc_forward": [vp, i64, i64, i64, vp, vp, vp, vp, i64, vp],
        "s3grl_gic_disc_backward": [vp, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp],
        "s3grl_wp_layout": [i64, i64, i32, i32, i64, C.POINTER(i64)],
        "s3grl_wp_attention_forward": [vp, C.POINTER(WpBatch), i32, i32, vp, vp, vp, vp, vp, vp],
        "s3grl_wp_attention_backward": [vp, C.POINTER(WpBatch), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "s3grl_wp_walk_forward": [vp, C.POINTER(WpBatch), i32, i32, i64, vp, vp, vp, i64, vp],
        "s3grl_wp_walk_backward": [vp, C.POINTER(WpBatch), i32, i32, i64, vp, vp, vp, vp, i64, vp, vp],
        "s3grl_candidates_layout": [i64, i32, C.POINTER(i64)],
        "s3grl_candidates_count": [vp, vp, vp, i64, i32, vp, i64, vp, C.POINTER(i64)],
        "s3grl_candidates_fill": [vp, vp, vp, i64, i32, vp, i64, vp, vp],
        "s3grl_segment_topk": [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp],
    }
    for name, args in proto.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = i32
    if L.s3grl_abi_version() != ABI_VERSION:
        raise ImportError("libs3grl_hip.so ABI version mismatch")
    _lib = L
    return L


def ptr(t):
    """The device (or host) address of a tensor's data as c_void_p; NULL for None and for an empty tensor."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


def aligned16(t):
    """t itself when its data starts on a 16-byte boundary, else a copy that does (a fresh allocation): the float4
    kernels read and write rows as 16-byte words.  Apply after .contiguous(), which keeps a contiguous view that
    starts anywhere in its buffer."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


_EXC = {
    ERR_NOT_IMPLEMENTED: NotImplementedError,   # reference tuned_SIGN.py:235,251; utils.py:553
    ERR_NO_FEATURES: AssertionError,            # reference tuned_SIGN.py:166,221
    ERR_INVALID_ARGUMENT: ValueError,
    ERR_SELF_LINK: ValueError,
    ERR_OUT_OF_MEMORY: MemoryError,
}


def check(status, what):
    """Map a status code onto the Python exception the reference would raise."""
    if status == OK:
        return
    L = lib()
    detail = L.s3grl_last_error().decode()
    name = L.s3grl_status_string(status).decode()
    exc = _EXC.get(status)
    msg = f"{what}: {name}" + (f" ({detail})" if detail else "")
    if exc is None:
        raise S3GRLError(status, f"{what}: {name}", detail)
    raise exc(msg)
