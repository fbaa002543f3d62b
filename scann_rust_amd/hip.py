"""Raw ctypes binding of libscann_hip.so (include/scann_hip.h).

Plumbing only: numpy arrays in, numpy arrays out.  There is NO fallback: if the
library is missing or no gfx950 device is present every call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCANN_HIP_LIB: alternative build of the same library (kernel-tuning sweeps)
LIB_PATH = os.environ.get("SCANN_HIP_LIB") or os.path.join(_HERE, "libscann_hip.so")

OK, INVALID_ARGUMENT, RESOURCE_EXHAUSTED, FAILED_PRECONDITION = 0, 3, 8, 9
NOT_FOUND, ABORTED = 5, 10
OUT_OF_RANGE, UNIMPLEMENTED, INTERNAL, UNAVAILABLE = 11, 12, 13, 14
SQUARED_L2, L2, DOT_PRODUCT, L1, COSINE = 0, 1, 2, 3, 4
MMR_MAX_DEPTH = 2048    # SCANN_HIP_MMR_MAX_DEPTH
CROWD_MAX_DIMS = 8      # SCANN_HIP_CROWD_MAX_DIMS
MUTABLE_MAX_CAPACITY = 65536   # SCANN_HIP_MUTABLE_MAX_CAPACITY
MUTABLE_MAX_K = 2048           # SCANN_HIP_MUTABLE_MAX_K
MUTABLE_DELTA_TILE = 1024      # SCANN_HIP_MUTABLE_DELTA_TILE: delta rows sorted per workgroup of the delta scan
FOLD_CHUNK = 1024              # SCANN_HIP_FOLD_CHUNK: CSR positions per workgroup of the fold's count and scatter passes
TOKEN_TILE_BITS = 65536        # SCANN_HIP_TOKEN_TILE_BITS: bits of one query's bitmap a workgroup of the token-map kernel assembles in LDS
ALLOW_AND, ALLOW_OR, ALLOW_ANDNOT, ALLOW_NOT = 1, 2, 3, 4   # SCANN_HIP_ALLOW_*: ops of allow_bitmaps_combine
ATTR_I64, ATTR_F32 = 1, 2      # SCANN_HIP_ATTR_*: column types of an AttrTable
ATTR_ROW_INDEX = 0xFFFFFFFF    # SCANN_HIP_ATTR_ROW_INDEX: the pseudo-column whose value at row j is j (RangeFilter)
ATTR_MAX_CLAUSES = 8           # SCANN_HIP_ATTR_MAX_CLAUSES: clauses of one range call
RANGE_TILE_BITS = 1024         # SCANN_HIP_RANGE_TILE_BITS: rows whose values a workgroup of the range kernel holds in registers

_CODE_NAMES = {
    0: "Ok", 1: "Cancelled", 2: "Unknown", 3: "InvalidArgument", 4: "DeadlineExceeded",
    5: "NotFound", 6: "AlreadyExists", 7: "PermissionDenied", 8: "ResourceExhausted",
    9: "FailedPrecondition", 10: "Aborted", 11: "OutOfRange", 12: "Unimplemented",
    13: "Internal", 14: "Unavailable", 15: "DataLoss", 16: "Unauthenticated",
}

EXPORTS = [
    "scann_hip_init", "scann_hip_shutdown", "scann_hip_last_error", "scann_hip_version",
    "scann_hip_compute_stride", "scann_hip_bf_create", "scann_hip_bf_create_quantized", "scann_hip_bf16_quantize",
    "scann_hip_txh_create", "scann_hip_txh_create_quantized", "scann_hip_index_device_bytes",
    "scann_hip_search_opts_default", "scann_hip_search_batched", "scann_hip_search_batched_params", "scann_hip_index_reserve",
    "scann_hip_search_batched_device", "scann_hip_index_last_device_status", "scann_hip_index_debug_filter_bounds",
    "scann_hip_index_debug_rerank_brackets", "scann_hip_index_debug_survivor_bitmap_bytes",
    "scann_hip_crowd_table_slots", "scann_hip_index_set_crowding_attributes", "scann_hip_search_crowded",
    "scann_hip_index_reserve_crowded", "scann_hip_search_crowded_device",
    "scann_hip_index_set_crowding_attributes_md", "scann_hip_search_crowded_md", "scann_hip_search_crowded_md_device",
    "scann_hip_crowd_md_apply",
    "scann_hip_search_mmr", "scann_hip_search_mmr_device", "scann_hip_index_reserve_mmr", "scann_hip_mmr_apply",
    "scann_hip_txh_search_local_device", "scann_hip_txh_merge_device",
    "scann_hip_assign_leaves", "scann_hip_txh_partition", "scann_hip_lut_from_query",
    "scann_hip_adc_distances", "scann_hip_lut16_distances_batch", "scann_hip_encode",
    "scann_hip_fp8_quantize", "scann_hip_fp8_dequantize", "scann_hip_fp8_distances",
    "scann_hip_bf_distances", "scann_hip_bf_search_radius", "scann_hip_bf_search_radius_opts", "scann_hip_allow_bitmap_count", "scann_hip_allow_bitmaps_from_ids", "scann_hip_allow_bitmaps_from_ids_device", "scann_hip_bf_assign_nearest",
    "scann_hip_kmeans_init_pp", "scann_hip_kmeans_lloyd", "scann_hip_txh_pack_blocks_device", "scann_hip_index_size", "scann_hip_index_dimensionality",
    "scann_hip_index_destroy", "scann_hip_index_enable_timing",
    "scann_hip_index_last_kernel_ms",
    "scann_hip_txh_write_file", "scann_hip_bf_write_file", "scann_hip_index_file_info",
    "scann_hip_index_load_file",
    "scann_hip_abi_layout", "scann_hip_lut16_quantize",
    "scann_hip_comm_unique_id", "scann_hip_comm_create", "scann_hip_comm_destroy",
    "scann_hip_txh_search_sharded_device", "scann_hip_comm_last_status", "scann_hip_comm_layout",
    "scann_hip_mutable_create", "scann_hip_mutable_destroy", "scann_hip_mutable_add", "scann_hip_mutable_remove",
    "scann_hip_mutable_update", "scann_hip_mutable_get", "scann_hip_mutable_exists", "scann_hip_mutable_size",
    "scann_hip_mutable_pending", "scann_hip_mutable_needs_rebuild", "scann_hip_mutable_search",
    "scann_hip_mutable_export_live", "scann_hip_mutable_rebase", "scann_hip_mutable_enable_timing",
    "scann_hip_mutable_last_stage_ms", "scann_hip_fold_mutable", "scann_hip_fold_mutable_stage_ms",
    "scann_hip_index_write_file",
    "scann_hip_token_map_create", "scann_hip_token_map_destroy", "scann_hip_token_map_num_tokens",
    "scann_hip_token_map_num_datapoints", "scann_hip_token_map_get_indices", "scann_hip_token_map_allow_bitmaps_device",
    "scann_hip_token_map_allow_bitmaps", "scann_hip_allow_bitmaps_from_tokens", "scann_hip_search_batched_tokens",
    "scann_hip_allow_bitmaps_combine", "scann_hip_allow_bitmaps_combine_device",
    "scann_hip_attr_table_create", "scann_hip_attr_table_destroy", "scann_hip_attr_table_num_datapoints",
    "scann_hip_attr_table_num_columns", "scann_hip_attr_table_column_type", "scann_hip_attr_table_allow_bitmaps_device",
    "scann_hip_attr_table_allow_bitmaps", "scann_hip_allow_bitmaps_from_ranges", "scann_hip_search_batched_ranges",
    "scann_hip_index_quantization_stats", "scann_hip_scalar_quantizer_calibrate", "scann_hip_scalar_quantize",
    "scann_hip_scalar_dequantize", "scann_hip_scalar_quantize_device", "scann_hip_index_quantize_rows",
    "scann_hip_projection_create", "scann_hip_projection_destroy", "scann_hip_projection_info", "scann_hip_project",
    "scann_hip_project_device", "scann_hip_txh_create_projected", "scann_hip_index_projection_info",
    "scann_hip_build_config_default", "scann_hip_txh_build",
    "scann_hip_pca_train", "scann_hip_projection_arrays", "scann_hip_pca_last_stage_ms", "scann_hip_txh_build_projected",
    "scann_hip_tree_config_default", "scann_hip_txh_build_hierarchical",
]


class ScannError(RuntimeError):
    """error.rs:73-147: ScannError { code, message }."""

    def __init__(self, code, message):
        super().__init__("%s: %s" % (_CODE_NAMES.get(code, str(code)), message))
        self.code = code
        self.message = message


f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u16p = C.POINTER(C.c_uint16)
u8p = C.POINTER(C.c_uint8)
i8p = C.POINTER(C.c_int8)
i32p = C.POINTER(C.c_int32)
vp = C.c_void_p


class TxhDesc(C.Structure):
    _fields_ = [
        ("data", f32p), ("n_rows", C.c_uint64), ("dim", C.c_uint32), ("stride", C.c_uint32),
        ("data_is_csr_order", C.c_int32),
        ("centers", f32p), ("num_partitions", C.c_uint32),
        ("leaf_offsets", u32p), ("leaf_ids", u32p), ("leaf_sizes_global", u32p),
        ("n_local", C.c_uint64),
        ("codebook", f32p), ("num_subspaces", C.c_uint32), ("num_codes", C.c_uint32),
        ("dims_per_subspace", C.c_uint32),
        ("codes", u8p), ("codes_packed4", C.c_int32), ("use_residuals", C.c_int32),
        ("partitions_to_search", C.c_uint32), ("pre_reorder_multiplier", C.c_float),
        ("distance_measure", C.c_int32),
    ]


class FileInfo(C.Structure):
    _fields_ = [
        ("version", C.c_uint32), ("kind", C.c_uint32),
        ("n_rows", C.c_uint64), ("n_local", C.c_uint64), ("file_bytes", C.c_uint64),
        ("dim", C.c_uint32), ("stride", C.c_uint32), ("num_partitions", C.c_uint32),
        ("num_subspaces", C.c_uint32), ("num_codes", C.c_uint32), ("dims_per_subspace", C.c_uint32),
        ("distance_measure", C.c_int32), ("data_is_csr_order", C.c_int32), ("codes_packed4", C.c_int32),
        ("use_residuals", C.c_int32), ("partitions_to_search", C.c_uint32),
        ("pre_reorder_multiplier", C.c_float), ("has_data", C.c_int32),
    ]


class SearchOpts(C.Structure):
    _fields_ = [
        ("partitions_to_search", C.c_uint32), ("pre_reorder_k", C.c_uint32),
        ("exact_reorder", C.c_int32),
        ("tokens", u32p), ("token_dists", f32p),
        ("cand_idx", u32p), ("cand_dist", f32p), ("cand_count", u32p),
        ("allow_bitmap", u64p), ("allow_bitmap_bits", C.c_uint64),
        ("bf_exact", C.c_int32),
        ("allow_bitmap_stride", C.c_uint64),
    ]


class BuildConfig(C.Structure):
    """scann_hip_build_config"""
    _fields_ = [
        ("num_partitions", C.c_uint32), ("kmeans_iterations", C.c_uint32), ("kmeans_convergence", C.c_double),
        ("kmeans_seed", C.c_uint64),
        ("num_subspaces", C.c_uint32), ("num_codes", C.c_uint32),
        ("training_iterations", C.c_uint32), ("convergence_threshold", C.c_double),
        ("seed", C.c_uint64),
        ("simd_threshold", C.c_uint32), ("use_residuals", C.c_int32), ("store_rows", C.c_int32),
        ("batched_codebook", C.c_int32),
        ("partitions_to_search", C.c_uint32), ("pre_reorder_multiplier", C.c_float), ("distance_measure", C.c_int32),
    ]


class BuildReport(C.Structure):
    """scann_hip_build_report"""
    _fields_ = [
        ("partition_iterations", C.c_uint32), ("partition_converged", C.c_int32), ("partition_inertia", C.c_double),
        ("subspace_iterations", C.c_uint32 * 64), ("subspace_converged", C.c_int32 * 64),
        ("stage_ms", C.c_float * 7),
    ]


class TreeConfig(C.Structure):
    """scann_hip_tree_config"""
    _fields_ = [
        ("num_children", C.c_uint32), ("max_depth", C.c_uint32), ("min_leaf_size", C.c_uint32),
        ("kmeans_iterations", C.c_uint32), ("kmeans_convergence", C.c_double), ("seed", C.c_uint64),
    ]


class TreeReport(C.Structure):
    """scann_hip_tree_report"""
    _fields_ = [
        ("num_leaves", C.c_uint32), ("depth_reached", C.c_uint32),
        ("level_nodes", C.c_uint32 * 5), ("level_iterations", C.c_uint32 * 5), ("level_converged", C.c_uint32 * 5),
        ("level_leaves", C.c_uint32 * 5),
        ("stage_ms", C.c_float * 10),
    ]


_lib = None


def load():
    """Load the shared library (no GPU needed just to load and look up symbols)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScannError(UNAVAILABLE, "libscann_hip.so is not built (run "
                         "`python -m scann_rust_amd.build`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    L.scann_hip_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.scann_hip_shutdown.argtypes = [vp]
    L.scann_hip_shutdown.restype = None
    L.scann_hip_last_error.restype = C.c_char_p
    L.scann_hip_version.restype = C.c_char_p
    L.scann_hip_compute_stride.restype = C.c_uint32
    L.scann_hip_compute_stride.argtypes = [C.c_uint32]
    L.scann_hip_bf_create.argtypes = [vp, f32p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
                                      C.POINTER(vp)]
    L.scann_hip_bf_create_quantized.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_float,
                                                C.c_int, C.POINTER(vp)]
    L.scann_hip_bf16_quantize.argtypes = [vp, f32p, C.c_uint64, u16p]
    L.scann_hip_txh_create.argtypes = [vp, C.POINTER(TxhDesc), C.POINTER(vp)]
    L.scann_hip_txh_create_quantized.argtypes = [vp, C.POINTER(TxhDesc), vp, C.c_int, C.c_float, C.POINTER(vp)]
    L.scann_hip_index_device_bytes.restype = C.c_uint64
    L.scann_hip_index_device_bytes.argtypes = [vp]
    L.scann_hip_txh_write_file.argtypes = [C.c_char_p, C.POINTER(TxhDesc)]
    L.scann_hip_bf_write_file.argtypes = [C.c_char_p, f32p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    L.scann_hip_index_file_info.argtypes = [C.c_char_p, C.POINTER(FileInfo)]
    L.scann_hip_index_load_file.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.scann_hip_search_opts_default.argtypes = [C.POINTER(SearchOpts)]
    L.scann_hip_search_opts_default.restype = None
    L.scann_hip_search_batched.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.POINTER(SearchOpts), u32p, f32p, u32p]
    L.scann_hip_search_batched_params.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                                                  C.POINTER(SearchOpts), C.c_uint32, u32p, f32p, u32p]
    L.scann_hip_index_reserve.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(SearchOpts)]
    L.scann_hip_search_batched_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.POINTER(SearchOpts), vp, vp, vp, vp]
    L.scann_hip_index_last_device_status.argtypes = [vp, vp]
    L.scann_hip_index_debug_filter_bounds.argtypes = [vp, vp, C.c_uint32, u64p]
    L.scann_hip_index_debug_survivor_bitmap_bytes.argtypes = [vp, vp, u64p]
    L.scann_hip_index_debug_rerank_brackets.argtypes = [vp, vp, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p]
    L.scann_hip_crowd_table_slots.restype = C.c_uint32
    L.scann_hip_crowd_table_slots.argtypes = [C.c_uint32]
    L.scann_hip_index_set_crowding_attributes.argtypes = [vp, u64p, C.c_uint64]
    L.scann_hip_search_crowded.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.POINTER(SearchOpts), u32p, f32p, u32p]
    L.scann_hip_index_reserve_crowded.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SearchOpts)]
    L.scann_hip_search_crowded_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.POINTER(SearchOpts), vp, vp, vp, vp]
    L.scann_hip_index_set_crowding_attributes_md.argtypes = [vp, u64p, C.c_uint32, C.c_uint64]
    L.scann_hip_search_crowded_md.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              u32p, C.c_uint32, C.POINTER(SearchOpts), u32p, f32p, u32p]
    L.scann_hip_search_crowded_md_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                                                     C.c_uint32, C.POINTER(SearchOpts), vp, vp, vp, vp]
    L.scann_hip_crowd_md_apply.argtypes = [vp, u32p, f32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32,
                                           u32p, f32p, u32p]
    L.scann_hip_search_mmr.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                       C.POINTER(SearchOpts), u32p, f32p, u32p]
    L.scann_hip_search_mmr_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                              C.POINTER(SearchOpts), vp, vp, vp, vp]
    L.scann_hip_index_reserve_mmr.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SearchOpts)]
    L.scann_hip_mmr_apply.argtypes = [vp, u32p, f32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                      u32p, f32p, u32p]
    L.scann_hip_txh_search_local_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.POINTER(SearchOpts), vp, vp, vp, vp, vp]
    L.scann_hip_txh_merge_device.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.scann_hip_assign_leaves.argtypes = [u32p, C.c_uint32, C.c_uint32, u32p]
    L.scann_hip_txh_partition.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_uint32, u32p, f32p, u32p]
    L.scann_hip_lut_from_query.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, u32p, f32p]
    L.scann_hip_adc_distances.argtypes = [vp, f32p, C.c_uint32, f32p]
    L.scann_hip_lut16_distances_batch.argtypes = [vp, u8p, u8p, C.c_uint32, C.c_uint64,
                                                  C.c_float, C.c_float, f32p]
    L.scann_hip_encode.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, f32p,
                                   C.c_uint64, C.c_uint32, f32p, u32p, u8p]
    L.scann_hip_bf_distances.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, f32p]
    L.scann_hip_bf_assign_nearest.argtypes = [vp, f32p, C.c_uint32, u32p, f32p]
    L.scann_hip_txh_pack_blocks_device.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp,
                                                   C.c_uint64, vp]
    L.scann_hip_kmeans_init_pp.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                           f32p]
    L.scann_hip_kmeans_lloyd.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, C.c_uint32, C.c_uint32,
                                         C.c_double, C.c_uint32, u32p, u32p, C.POINTER(C.c_double), u32p,
                                         C.POINTER(C.c_int)]
    L.scann_hip_build_config_default.argtypes = [C.POINTER(BuildConfig)]
    L.scann_hip_build_config_default.restype = None
    L.scann_hip_txh_build.argtypes = [vp, C.POINTER(BuildConfig), C.POINTER(vp), C.POINTER(BuildReport)]
    L.scann_hip_tree_config_default.argtypes = [C.POINTER(TreeConfig)]
    L.scann_hip_tree_config_default.restype = None
    L.scann_hip_txh_build_hierarchical.argtypes = [vp, C.POINTER(TreeConfig), C.POINTER(BuildConfig), C.POINTER(vp),
                                                   C.POINTER(BuildReport), C.POINTER(TreeReport)]
    L.scann_hip_abi_layout.restype = C.c_uint32
    L.scann_hip_abi_layout.argtypes = [u32p, C.c_uint32]
    L.scann_hip_lut16_quantize.argtypes = [vp, f32p, C.c_uint32, u8p, f32p, f32p]
    L.scann_hip_fp8_quantize.argtypes = [vp, f32p, C.c_uint64, C.c_float, C.c_int, u8p]
    L.scann_hip_fp8_dequantize.argtypes = [vp, u8p, C.c_uint64, C.c_float, C.c_int, f32p]
    L.scann_hip_fp8_distances.argtypes = [vp, f32p, C.c_uint32, u8p, C.c_uint64, C.c_uint64, C.c_int, f32p]
    L.scann_hip_comm_unique_id.argtypes = [vp]
    L.scann_hip_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.scann_hip_comm_destroy.argtypes = [vp]
    L.scann_hip_comm_destroy.restype = None
    L.scann_hip_txh_search_sharded_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                                      C.POINTER(SearchOpts), C.c_uint32, vp, vp, vp, vp]
    L.scann_hip_comm_last_status.argtypes = [vp]
    L.scann_hip_comm_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p]
    L.scann_hip_bf_search_radius.argtypes = [vp, f32p, C.c_uint32, C.c_float, u32p, f32p, C.c_uint64,
                                             C.POINTER(C.c_uint64)]
    L.scann_hip_bf_search_radius_opts.argtypes = [vp, f32p, C.c_uint32, C.c_float, C.POINTER(SearchOpts), u32p, f32p,
                                                  C.c_uint64, C.POINTER(C.c_uint64)]
    L.scann_hip_allow_bitmap_count.restype = C.c_uint64
    L.scann_hip_allow_bitmap_count.argtypes = [u64p, C.c_uint64, C.c_uint64]
    L.scann_hip_allow_bitmaps_from_ids.argtypes = [u32p, u64p, C.c_uint32, C.c_uint64, C.c_uint64, u64p]
    L.scann_hip_allow_bitmaps_from_ids_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp]
    L.scann_hip_index_size.restype = C.c_uint64
    L.scann_hip_index_size.argtypes = [vp]
    L.scann_hip_index_dimensionality.restype = C.c_uint32
    L.scann_hip_index_dimensionality.argtypes = [vp]
    L.scann_hip_index_destroy.argtypes = [vp]
    L.scann_hip_index_destroy.restype = None
    L.scann_hip_index_enable_timing.argtypes = [vp, C.c_int]
    L.scann_hip_index_enable_timing.restype = None
    L.scann_hip_index_last_kernel_ms.restype = C.c_float
    L.scann_hip_index_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.scann_hip_mutable_create.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp)]
    L.scann_hip_mutable_destroy.argtypes = [vp]
    L.scann_hip_mutable_destroy.restype = None
    L.scann_hip_mutable_add.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    L.scann_hip_mutable_remove.argtypes = [vp, u32p, C.c_uint32]
    L.scann_hip_mutable_update.argtypes = [vp, u32p, f32p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.scann_hip_mutable_get.argtypes = [vp, C.c_uint32, f32p]
    L.scann_hip_mutable_exists.argtypes = [vp, C.c_uint32]
    L.scann_hip_mutable_size.restype = C.c_uint64
    L.scann_hip_mutable_size.argtypes = [vp]
    L.scann_hip_mutable_pending.restype = C.c_uint64
    L.scann_hip_mutable_pending.argtypes = [vp]
    L.scann_hip_mutable_needs_rebuild.argtypes = [vp, C.c_uint64]
    L.scann_hip_mutable_search.argtypes = [vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.POINTER(SearchOpts), u32p, f32p, u32p]
    L.scann_hip_mutable_export_live.argtypes = [vp, f32p, u32p, C.c_uint64, u64p]
    L.scann_hip_mutable_rebase.argtypes = [vp, vp, u32p, C.c_uint64]
    L.scann_hip_mutable_enable_timing.argtypes = [vp, C.c_int]
    L.scann_hip_mutable_enable_timing.restype = None
    L.scann_hip_mutable_last_stage_ms.argtypes = [vp, f32p]
    L.scann_hip_fold_mutable.argtypes = [vp, C.POINTER(vp), u32p, C.c_uint64, u64p]
    L.scann_hip_fold_mutable_stage_ms.argtypes = [vp, f32p]
    L.scann_hip_index_write_file.argtypes = [vp, C.c_char_p]
    L.scann_hip_token_map_create.argtypes = [vp, C.c_uint64, u32p, u64p, C.c_uint64, C.POINTER(vp)]
    L.scann_hip_token_map_destroy.argtypes = [vp]
    L.scann_hip_token_map_destroy.restype = None
    L.scann_hip_token_map_num_tokens.restype = C.c_uint64
    L.scann_hip_token_map_num_tokens.argtypes = [vp]
    L.scann_hip_token_map_num_datapoints.restype = C.c_uint64
    L.scann_hip_token_map_num_datapoints.argtypes = [vp]
    L.scann_hip_token_map_get_indices.argtypes = [vp, C.c_uint64, u32p, C.c_uint64, u64p]
    L.scann_hip_token_map_allow_bitmaps_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp]
    L.scann_hip_token_map_allow_bitmaps.argtypes = [vp, u64p, u64p, C.c_uint32, C.c_uint64, u64p]
    L.scann_hip_allow_bitmaps_from_tokens.argtypes = [u32p, u64p, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint32,
                                                      C.c_uint64, u64p]
    L.scann_hip_search_batched_tokens.argtypes = [vp, vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.POINTER(SearchOpts), u64p, u64p, u32p, f32p, u32p]
    L.scann_hip_allow_bitmaps_combine.argtypes = [C.c_int, u64p, C.c_uint64, u64p, C.c_uint64, C.c_uint32, C.c_uint64,
                                                  u64p, C.c_uint64]
    L.scann_hip_allow_bitmaps_combine_device.argtypes = [vp, C.c_int, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32,
                                                         C.c_uint64, vp, C.c_uint64, vp]
    L.scann_hip_attr_table_create.argtypes = [vp, C.c_uint64, C.c_uint32, i32p, C.POINTER(vp), C.POINTER(vp)]
    L.scann_hip_attr_table_destroy.argtypes = [vp]
    L.scann_hip_attr_table_destroy.restype = None
    L.scann_hip_attr_table_num_datapoints.restype = C.c_uint64
    L.scann_hip_attr_table_num_datapoints.argtypes = [vp]
    L.scann_hip_attr_table_num_columns.restype = C.c_uint32
    L.scann_hip_attr_table_num_columns.argtypes = [vp]
    L.scann_hip_attr_table_column_type.argtypes = [vp, C.c_uint32]
    L.scann_hip_attr_table_allow_bitmaps_device.argtypes = [vp, u32p, C.c_uint32, vp, C.c_uint32, C.c_int, C.c_uint64, vp, vp]
    L.scann_hip_attr_table_allow_bitmaps.argtypes = [vp, u32p, C.c_uint32, u64p, C.c_uint32, C.c_int, C.c_uint64, u64p]
    L.scann_hip_allow_bitmaps_from_ranges.argtypes = [C.c_uint64, C.c_uint32, i32p, C.POINTER(vp), u32p, C.c_uint32, u64p,
                                                      C.c_uint32, C.c_int, C.c_uint64, u64p]
    L.scann_hip_search_batched_ranges.argtypes = [vp, vp, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.POINTER(SearchOpts), u32p, C.c_uint32, u64p, u32p, f32p, u32p]
    L.scann_hip_index_quantization_stats.argtypes = [vp, f32p]
    L.scann_hip_scalar_quantizer_calibrate.argtypes = [f32p, C.c_uint32, C.c_int, C.c_float, C.c_float, f32p, i32p]
    L.scann_hip_scalar_quantize.argtypes = [f32p, C.c_uint64, C.c_uint32, C.c_int, f32p, i8p]
    L.scann_hip_scalar_dequantize.argtypes = [i8p, C.c_uint64, C.c_int, f32p, f32p]
    L.scann_hip_scalar_quantize_device.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, f32p,
                                                   vp, C.c_uint32, vp]
    L.scann_hip_index_quantize_rows.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_float, C.POINTER(vp),
                                                f32p, i32p]
    L.scann_hip_projection_create.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, f32p, f32p, C.c_uint32, C.POINTER(vp)]
    L.scann_hip_projection_destroy.argtypes = [vp]
    L.scann_hip_projection_destroy.restype = None
    L.scann_hip_projection_info.argtypes = [vp, u32p]
    L.scann_hip_project.argtypes = [vp, f32p, C.c_uint64, C.c_uint32, C.c_uint32, f32p, C.c_uint32]
    L.scann_hip_project_device.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp]
    L.scann_hip_txh_create_projected.argtypes = [vp, C.POINTER(TxhDesc), vp, f32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                 C.POINTER(vp)]
    L.scann_hip_index_projection_info.argtypes = [vp, u32p]
    L.scann_hip_pca_train.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), u32p, C.POINTER(C.c_int)]
    L.scann_hip_projection_arrays.argtypes = [vp, f32p, f32p]
    L.scann_hip_pca_last_stage_ms.argtypes = [f32p]
    L.scann_hip_pca_last_stage_ms.restype = None
    L.scann_hip_txh_build_projected.argtypes = [vp, vp, C.POINTER(BuildConfig), C.POINTER(vp), C.POINTER(BuildReport)]
    _lib = L
    return L


def check(status):
    if status != OK:
        raise ScannError(status, (load().scann_hip_last_error() or b"").decode())


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def ptr(a, ty):
    return a.ctypes.data_as(ty) if a is not None else None


_ctx = {}


def context(device=0):
    """Process-wide context per device (scann_hip_init)."""
    if device not in _ctx:
        h = vp()
        check(load().scann_hip_init(device, C.byref(h)))
        _ctx[device] = h
    return _ctx[device]


def compute_stride(dim):
    return int(load().scann_hip_compute_stride(dim))


def default_opts():
    o = SearchOpts()
    load().scann_hip_search_opts_default(C.byref(o))
    return o


class Index:
    """Owns one scann_hip_index handle."""

    def __init__(self, handle, keep=()):
        self.h = handle
        self._keep = keep

    def close(self):
        if self.h:
            load().scann_hip_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return int(load().scann_hip_index_size(self.h))

    def dimensionality(self):
        return int(load().scann_hip_index_dimensionality(self.h))

    def projection_info(self):
        """(kind, in_dim, out_dim, start) of the projection the handle searches through; kind 0 on any other handle
        (scann_hip_index_projection_info)."""
        out = np.zeros(4, np.uint32)
        check(load().scann_hip_index_projection_info(self.h, ptr(out, u32p)))
        return tuple(int(v) for v in out)

    def device_bytes(self):
        """Bytes of the handle's persistent device allocations, search workspaces excluded
        (scann_hip_index_device_bytes)."""
        return int(load().scann_hip_index_device_bytes(self.h))

    def search_batched(self, queries, k, opts=None, q_dim=None, stages=False, allow=None, allow_bits=None):
        """`allow`: optional uint64 allow-bitmap (see allow_bitmap()) = search_with_filter.  `allow_bits`: its
        capacity in bits (default: every word, allow.size * 64); indices at or past it are not allowed.  A 2-D
        `allow` [nq, words] is one bitmap per query (allow_bitmap_stride = words; see allow_bitmaps_from_ids());
        `allow_bits` is then the capacity every row shares (default words * 64)."""
        q = f32(queries)
        if q.ndim == 1:
            q = q[None]
        nq, qs = q.shape
        qd = qs if q_dim is None else q_dim
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        o = opts if opts is not None else default_opts()
        extra = None
        if allow is not None:
            allow = _bind_allow(o, allow, allow_bits, nq)
        if stages:
            P = o.partitions_to_search or 4096
            m = o.pre_reorder_k or 4096
            tok = np.zeros((nq, P), np.uint32); tokd = np.zeros((nq, P), np.float32)
            ci = np.zeros((nq, m), np.uint32); cd = np.zeros((nq, m), np.float32)
            cc = np.zeros(nq, np.uint32)
            o.tokens, o.token_dists = ptr(tok, u32p), ptr(tokd, f32p)
            o.cand_idx, o.cand_dist, o.cand_count = ptr(ci, u32p), ptr(cd, f32p), ptr(cc, u32p)
            extra = (tok, tokd, ci, cd, cc)
        try:
            check(load().scann_hip_search_batched(self.h, ptr(q, f32p), nq, qs, qd, k, C.byref(o),
                                                  ptr(out_idx, u32p), ptr(out_dist, f32p),
                                                  ptr(out_cnt, u32p)))
        finally:
            # the caller's opts must not keep pointers into this call's arrays: a later call with the same opts
            # would write its stage outputs / read its filter through them
            if stages:
                o.tokens = o.token_dists = o.cand_idx = o.cand_dist = o.cand_count = None
            if allow is not None:
                o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
        if stages:
            return out_idx[:, :k], out_dist[:, :k], out_cnt, extra
        return out_idx[:, :k], out_dist[:, :k], out_cnt

    def search_batched_with_params(self, queries, ks, opts=None, allow=None, allow_bits=None):
        """Searcher::search_batched_with_params: one num_neighbors per query; rows at pitch max(ks).  `allow`,
        `allow_bits`: an allow-bitmap and its capacity, as in search_batched."""
        q = f32(queries)
        nq, qs = q.shape
        ks = np.ascontiguousarray(ks, np.uint32)
        pitch = max(int(ks.max()), 1)
        out_idx = np.zeros((nq, pitch), np.uint32); out_dist = np.zeros((nq, pitch), np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        if allow is not None:
            if opts is None:
                opts = default_opts()
            allow = _bind_allow(opts, allow, allow_bits, nq)
        try:
            check(load().scann_hip_search_batched_params(self.h, ptr(q, f32p), nq, qs, qs, ptr(ks, u32p),
                                                         C.byref(opts) if opts is not None else None, pitch,
                                                         ptr(out_idx, u32p), ptr(out_dist, f32p), ptr(out_cnt, u32p)))
        finally:
            if allow is not None:   # (see search_batched)
                opts.allow_bitmap, opts.allow_bitmap_bits, opts.allow_bitmap_stride = None, 0, 0
        return out_idx, out_dist, out_cnt

    def set_crowding_attributes(self, attrs):
        """One uint64 crowding attribute per datapoint index (the array may be shorter than the index: missing
        entries read as 0); None or an empty array detaches them.  scann_hip_index_set_crowding_attributes."""
        a = np.zeros(0, np.uint64) if attrs is None else np.ascontiguousarray(attrs, np.uint64).ravel()
        check(load().scann_hip_index_set_crowding_attributes(self.h, ptr(a, u64p) if a.size else None, a.size))

    def search_crowded(self, queries, k, depth, limit, opts=None, allow=None, allow_bits=None, q_dim=None):
        """CrowdingConstraint::apply(search(query, depth), k) with per_crowd_limit = `limit`, on the device
        (scann_hip_search_crowded).  depth = 0 means k.  `allow`, `allow_bits` as in search_batched."""
        q = f32(queries)
        if q.ndim == 1:
            q = q[None]
        nq, qs = q.shape
        qd = qs if q_dim is None else q_dim
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        o = opts if opts is not None else default_opts()
        if allow is not None:
            allow = _bind_allow(o, allow, allow_bits, nq)
        try:
            check(load().scann_hip_search_crowded(self.h, ptr(q, f32p), nq, qs, qd, k, depth, limit, C.byref(o),
                                                  ptr(out_idx, u32p), ptr(out_dist, f32p), ptr(out_cnt, u32p)))
        finally:
            if allow is not None:   # (see search_batched)
                o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
        return out_idx[:, :k], out_dist[:, :k], out_cnt

    def search_crowded_exact(self, query, k, limit, opts=None):
        """Brute-force handles: the crowded k nearest neighbours over the WHOLE index, one query.  Starts at
        depth = k and doubles it until the row holds k entries or depth has reached min(N, 2048).  Returns
        ((idx, dist), complete): complete is True when k were kept or the whole index was walked -- by the prefix
        property the answer then equals the rule applied to the full sorted database."""
        n = self.size()
        cap = min(n, 2048)
        depth = max(1, min(k, cap))
        while True:
            i, d, c = self.search_crowded(query, min(k, depth), depth, limit, opts=opts)
            c = int(c[0])
            if c >= k or depth >= cap:
                return (i[0, :c].copy(), d[0, :c].copy()), bool(c >= k or depth >= n)
            depth = min(2 * depth, cap)

    # ---- multi-attribute crowding and MMR (include/scann_hip.h) ----
    def _staged_host(self, call, queries, k, opts, allow, allow_bits, q_dim):
        """shared frame of the host entries of the stages: call(q_ptr, nq, q_stride, q_dim, opts_ref, oi, od, oc)"""
        q = f32(queries)
        if q.ndim == 1:
            q = q[None]
        nq, qs = q.shape
        qd = qs if q_dim is None else q_dim
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        o = opts if opts is not None else default_opts()
        if allow is not None:
            allow = _bind_allow(o, allow, allow_bits, nq)
        try:
            check(call(ptr(q, f32p), nq, qs, qd, C.byref(o), ptr(out_idx, u32p), ptr(out_dist, f32p), ptr(out_cnt, u32p)))
        finally:
            if allow is not None:   # (see search_batched)
                o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
        return out_idx[:, :k], out_dist[:, :k], out_cnt

    @staticmethod
    def _staged_apply(call, rows_idx, rows_dist, rows_count, k):
        """shared frame of the *_apply entries: call(ri, rd, rc, nq, depth, oi, od, oc); rows [nq][depth]"""
        ri = np.ascontiguousarray(rows_idx, np.uint32)
        rd = np.ascontiguousarray(rows_dist, np.float32)
        rc = np.ascontiguousarray(rows_count, np.uint32)
        nq, depth = ri.shape
        assert rd.shape == ri.shape and rc.shape == (nq,)
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        check(call(ptr(ri, u32p), ptr(rd, f32p), ptr(rc, u32p), nq, depth, ptr(out_idx, u32p), ptr(out_dist, f32p),
                   ptr(out_cnt, u32p)))
        return out_idx[:, :k], out_dist[:, :k], out_cnt

    def set_crowding_attributes_md(self, attrs, n_dims=None):
        """[n_dims][n_attrs] uint64 attributes, dimension-major (a 2-D array; n_dims only for an empty one); None or
        n_attrs = 0 detaches them.  scann_hip_index_set_crowding_attributes_md."""
        a = np.zeros((1, 0), np.uint64) if attrs is None else np.ascontiguousarray(attrs, np.uint64)
        if a.ndim != 2:
            raise ValueError("attrs must be [n_dims][n_attrs]")
        nd = a.shape[0] if n_dims is None else int(n_dims)
        check(load().scann_hip_index_set_crowding_attributes_md(self.h, ptr(a, u64p) if a.size else None, nd, a.shape[1]))

    def search_crowded_md(self, queries, k, depth, limits, opts=None, allow=None, allow_bits=None, q_dim=None):
        """CrowdingMultidimensional::apply(search(query, depth), k) with one limit per attribute dimension, on the
        device (scann_hip_search_crowded_md).  depth = 0 means k."""
        lim = np.ascontiguousarray(limits, np.uint32).ravel()
        return self._staged_host(
            lambda q, nq, qs, qd, o, oi, od, oc: load().scann_hip_search_crowded_md(
                self.h, q, nq, qs, qd, k, depth, ptr(lim, u32p), lim.size, o, oi, od, oc),
            queries, k, opts, allow, allow_bits, q_dim)

    def search_crowded_md_device(self, d_queries, nq, q_stride, k, depth, limits, d_out_idx, d_out_dist, d_out_count,
                                 stream, opts=None):
        """scann_hip_search_crowded_md_device: device addresses (integers) and a HIP stream handle; enqueue only"""
        lim = np.ascontiguousarray(limits, np.uint32).ravel()
        check(load().scann_hip_search_crowded_md_device(
            self.h, vp(d_queries), nq, q_stride, k, depth, ptr(lim, u32p), lim.size,
            C.byref(opts) if opts is not None else None, vp(d_out_idx), vp(d_out_dist), vp(d_out_count), vp(stream)))

    def crowd_md_apply(self, rows_idx, rows_dist, rows_count, k, limits):
        """CrowdingMultidimensional::apply on the caller's rows [nq][depth] (scann_hip_crowd_md_apply)"""
        lim = np.ascontiguousarray(limits, np.uint32).ravel()
        return self._staged_apply(
            lambda ri, rd, rc, nq, depth, oi, od, oc: load().scann_hip_crowd_md_apply(
                self.h, ri, rd, rc, nq, depth, k, ptr(lim, u32p), lim.size, oi, od, oc),
            rows_idx, rows_dist, rows_count, k)

    def search_mmr(self, queries, k, depth, lam, opts=None, allow=None, allow_bits=None, q_dim=None):
        """MmrDiversifier::new(lam).apply(search(query, depth), k, sim) with sim = minus the handle's distance between
        two stored rows, on the device (scann_hip_search_mmr).  Rows come back in selection order."""
        return self._staged_host(
            lambda q, nq, qs, qd, o, oi, od, oc: load().scann_hip_search_mmr(
                self.h, q, nq, qs, qd, k, depth, C.c_float(lam), o, oi, od, oc),
            queries, k, opts, allow, allow_bits, q_dim)

    def search_mmr_device(self, d_queries, nq, q_stride, k, depth, lam, d_out_idx, d_out_dist, d_out_count, stream,
                          opts=None):
        """scann_hip_search_mmr_device: device addresses (integers) and a HIP stream handle; enqueue only"""
        check(load().scann_hip_search_mmr_device(
            self.h, vp(d_queries), nq, q_stride, k, depth, C.c_float(lam), C.byref(opts) if opts is not None else None,
            vp(d_out_idx), vp(d_out_dist), vp(d_out_count), vp(stream)))

    def reserve_mmr(self, max_nq, max_k, max_depth=0, opts=None):
        check(load().scann_hip_index_reserve_mmr(self.h, max_nq, max_k, max_depth,
                                                 C.byref(opts) if opts is not None else None))

    def mmr_apply(self, rows_idx, rows_dist, rows_count, k, lam):
        """MmrDiversifier::apply on the caller's rows [nq][depth] (scann_hip_mmr_apply)"""
        return self._staged_apply(
            lambda ri, rd, rc, nq, depth, oi, od, oc: load().scann_hip_mmr_apply(
                self.h, ri, rd, rc, nq, depth, k, C.c_float(lam), oi, od, oc),
            rows_idx, rows_dist, rows_count, k)

    def search_radius(self, query, radius, capacity=None, allow=None, allow_bits=None):
        """Brute-force handles: bf_search_radius, with an optional allow-bitmap."""
        return bf_search_radius(self, query, radius, capacity, allow=allow, allow_bits=allow_bits)

    def enable_timing(self, on=True):
        load().scann_hip_index_enable_timing(self.h, 1 if on else 0)

    def last_kernel_ms(self):
        name = C.c_char_p()
        ms = load().scann_hip_index_last_kernel_ms(self.h, C.byref(name))
        return float(ms), (name.value or b"").decode()

    def debug_filter_bounds(self, nq, stream=0):
        """The filter bounds (uint64 merge keys, all ones = none) of the last batched search enqueued on `stream`
        (a HIP stream handle), which the caller has synchronised.  scann_hip_index_debug_filter_bounds."""
        out = np.zeros(nq, np.uint64)
        check(load().scann_hip_index_debug_filter_bounds(self.h, vp(stream), nq, ptr(out, u64p)))
        return out

    def debug_survivor_bitmap_bytes(self, stream=0):
        """bytes of survivor bitmaps the searches enqueued on `stream` have asked for (0: none of them took the sparse
        prefilter's bitmap form).  scann_hip_index_debug_survivor_bitmap_bytes."""
        out = C.c_uint64(0)
        check(load().scann_hip_index_debug_survivor_bitmap_bytes(self.h, vp(stream), C.byref(out)))
        return int(out.value)

    def debug_rerank_brackets(self, nq, m, stream=0):
        """(lb, ub, rows, counts) of the 8-bit row filter after the last batched search of nq queries with
        pre_reorder_k = m enqueued on `stream` (a HIP stream handle), which the caller has synchronised: ordered u32
        bounds [nq, m], re-rank rows [nq, m], candidates per query [nq] (0x80000000 where the shortlist kernel finished
        the query itself).  scann_hip_index_debug_rerank_brackets."""
        lb, ub, rows = (np.zeros((nq, m), np.uint32) for _ in range(3))
        counts = np.zeros(nq, np.uint32)
        check(load().scann_hip_index_debug_rerank_brackets(self.h, vp(stream), nq, m, ptr(lb, u32p), ptr(ub, u32p),
                                                           ptr(rows, u32p), ptr(counts, u32p)))
        return lb, ub, rows, counts


    def quantize_rows(self, fmt, mode=None, bits=8, num_std_devs=3.0, value_range=None):
        """A NEW Index over this handle's f32 rows stored as `fmt` (ROWS_BF16, ROWS_FP8_E4M3, ROWS_INT8), made on the
        device (scann_hip_index_quantize_rows); this handle stays as it is.  INT8: `mode` (default SQ_SIGNED, the mode
        whose codes mean what the searcher reads; SQ_STDDEV / SQ_SYMMETRIC / SQ_RANGE reproduce the reference,
        offset-binary bytes read as signed included), `bits`, `num_std_devs` (SQ_STDDEV), `value_range` = (min, max)
        (SQ_RANGE).  Returns (Index, params): params = {min, max, scale, inv_scale, zero_point}."""
        mode = SQ_SIGNED if mode is None else mode
        a, b = _sq_ab(mode, num_std_devs, value_range)
        h = vp()
        params = np.zeros(4, np.float32)
        zp = C.c_int32(0)
        check(load().scann_hip_index_quantize_rows(self.h, int(fmt), int(bits), int(mode), a, b, C.byref(h),
                                                   ptr(params, f32p), C.byref(zp)))
        return Index(h), _sq_params(params, zp.value)


class Mutable:
    """Owns one scann_hip_mutable handle over a base Index (kept alive here): MutableDataset + the rebuild counter of
    IncrementalUpdater (mutator/mod.rs) on the device.  Ids are u32 and stable; every mutation takes one row / id or a
    batch of them (applied in order, all or nothing)."""

    def __init__(self, base, capacity, device=0):
        h = vp()
        check(load().scann_hip_mutable_create(context(device), base.h, int(capacity), C.byref(h)))
        self.h = h
        self.base = base
        self.dim = base.dimensionality()
        self.stride = compute_stride(self.dim)

    def close(self):
        if self.h:
            load().scann_hip_mutable_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _rows(rows):
        r = f32(rows)
        return r[None] if r.ndim == 1 else r

    def add(self, rows):
        """one row -> its id; [n][dim] rows -> uint32 ids"""
        r = self._rows(rows)
        ids = np.zeros(r.shape[0], np.uint32)
        check(load().scann_hip_mutable_add(self.h, ptr(r, f32p), r.shape[0], r.shape[1], r.shape[1], ptr(ids, u32p)))
        return int(ids[0]) if np.ndim(rows) == 1 else ids

    def remove(self, ids):
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint32)
        check(load().scann_hip_mutable_remove(self.h, ptr(i, u32p), i.size))

    def update(self, ids, rows):
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint32)
        r = self._rows(rows)
        if r.shape[0] != i.size:
            raise ValueError("update: %d ids, %d rows" % (i.size, r.shape[0]))
        check(load().scann_hip_mutable_update(self.h, ptr(i, u32p), ptr(r, f32p), i.size, r.shape[1], r.shape[1]))

    def get(self, id):
        out = np.zeros(self.dim, np.float32)
        check(load().scann_hip_mutable_get(self.h, int(id), ptr(out, f32p)))
        return out

    def exists(self, id):
        return bool(load().scann_hip_mutable_exists(self.h, int(id)))

    def size(self):
        return int(load().scann_hip_mutable_size(self.h))

    def pending(self):
        return int(load().scann_hip_mutable_pending(self.h))

    def needs_rebuild(self, threshold):
        return bool(load().scann_hip_mutable_needs_rebuild(self.h, int(threshold)))

    def search_batched(self, queries, k, opts=None, allow=None, allow_bits=None):
        """out_idx holds external ids; `allow` is a uint64 bitmap over external ids, `allow_bits` its capacity"""
        q = f32(queries)
        if q.ndim == 1:
            q = q[None]
        nq, qs = q.shape
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        o = default_opts()
        if opts is not None:        # a copy: the caller's opts (and a filter it carries) are left as they are
            C.memmove(C.byref(o), C.byref(opts), C.sizeof(SearchOpts))
        if allow is not None:
            allow = np.ascontiguousarray(allow, np.uint64)
            o.allow_bitmap, o.allow_bitmap_bits = ptr(allow, u64p), _allow_capacity(allow, allow_bits)
        check(load().scann_hip_mutable_search(self.h, ptr(q, f32p), nq, qs, qs, k, C.byref(o), ptr(out_idx, u32p),
                                              ptr(out_dist, f32p), ptr(out_cnt, u32p)))
        return out_idx[:, :k], out_dist[:, :k], out_cnt

    def export_live(self):
        """(rows [n][dim], ids [n]) of every live row, ascending by id"""
        n = self.size()
        rows = np.zeros((max(n, 1), self.stride), np.float32)
        ids = np.zeros(max(n, 1), np.uint32)
        got = C.c_uint64(0)
        check(load().scann_hip_mutable_export_live(self.h, ptr(rows, f32p), ptr(ids, u32p), rows.shape[0], C.byref(got)))
        return np.ascontiguousarray(rows[:got.value, :self.dim]), ids[:got.value]

    def rebase(self, new_base, base_ids=None):
        """swap in `new_base`, whose row j has external id base_ids[j] (None = identity); the old base is released"""
        b = None if base_ids is None else np.ascontiguousarray(base_ids, np.uint32)
        check(load().scann_hip_mutable_rebase(self.h, new_base.h, ptr(b, u32p), new_base.size()))
        self.base = new_base

    def fold(self):
        """Fold the delta and the tombstones into a new base ON THE DEVICE, keeping the trained model, and rebase onto
        it (scann_hip_fold_mutable).  Returns (new base Index, base_ids): new datapoint j is the live row of id
        base_ids[j].  The old base is released once nothing else holds it."""
        n = self.size()
        ids = np.zeros(max(n, 1), np.uint32)
        got = C.c_uint64(0)
        h = vp()
        check(load().scann_hip_fold_mutable(self.h, C.byref(h), ptr(ids, u32p), ids.size, C.byref(got)))
        new_base = Index(h)
        self.base = new_base
        return new_base, ids[:got.value]

    def fold_stage_ms(self):
        """ms of (row gather, delta assign + encode, count + scans, scatter, finish half) of the last fold"""
        out = np.zeros(5, np.float32)
        check(load().scann_hip_fold_mutable_stage_ms(self.h, ptr(out, f32p)))
        return tuple(float(x) for x in out)

    def enable_timing(self, on=True):
        load().scann_hip_mutable_enable_timing(self.h, 1 if on else 0)

    def last_stage_ms(self):
        """HIP-event ms of (base pass, delta scan, merge) of the last three-stage search"""
        out = np.zeros(3, np.float32)
        check(load().scann_hip_mutable_last_stage_ms(self.h, ptr(out, f32p)))
        return tuple(float(x) for x in out)


def _allow_capacity(allow, allow_bits):
    """allow_bitmap_bits of a bitmap of allow.size words (2-D: of each row's words): every word, or the caller's
    capacity (at most that)"""
    words = allow.shape[-1] if allow.ndim == 2 else allow.size
    if allow_bits is None:
        return words * 64
    if not 0 <= int(allow_bits) <= words * 64:
        raise ValueError("allow_bits %d exceeds the bitmap's %d words" % (allow_bits, words))
    return int(allow_bits)


def _bind_allow(o, allow, allow_bits, nq):
    """Points the opts at an allow-bitmap for one call and returns the array the pointer reads (keep it alive across
    the call).  1-D: one bitmap for the batch.  2-D [nq, words]: one bitmap per query, its row pitch the stride."""
    allow = np.ascontiguousarray(allow, np.uint64)
    if allow.ndim == 2:
        if allow.shape[0] != nq:
            raise ValueError("a 2-D allow block needs one row per query: %d rows, %d queries" % (allow.shape[0], nq))
        o.allow_bitmap_stride = allow.shape[1]
        if allow.shape[1] == 0:   # (no words: capacity 0, nothing allowed; the library needs a non-null pointer)
            allow = np.zeros((nq, 1), np.uint64)
            o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = ptr(allow, u64p), 0, 0
            return allow
    elif allow.ndim != 1:
        raise ValueError("allow must be a 1-D bitmap or a 2-D [nq, words] block")
    else:
        o.allow_bitmap_stride = 0
    o.allow_bitmap, o.allow_bitmap_bits = ptr(allow, u64p), _allow_capacity(allow, allow_bits)
    return allow


def crowd_table_slots(depth):
    """slots of the crowding kernel's LDS attribute table for rows of `depth` entries (no GPU needed)"""
    return int(load().scann_hip_crowd_table_slots(int(depth)))


def allow_bitmap_count(allow, allow_bits, n):
    """rows of an n-row index the bitmap allows (set bits below min(allow_bits, n)): the host-side count a filtered
    brute-force search is planned with"""
    allow = np.ascontiguousarray(allow, np.uint64)
    return int(load().scann_hip_allow_bitmap_count(ptr(allow, u64p), _allow_capacity(allow, allow_bits), int(n)))


def allow_bitmaps_from_ids(ids, offsets, bits, stride_words=None):
    """[nq, stride_words] uint64 block of per-query allow-bitmaps of capacity `bits` from id lists: query i's ids are
    ids[offsets[i]:offsets[i + 1]] (RestrictAllowlist::from_indices per query; ids at or past `bits` are ignored,
    duplicates and any order are fine).  stride_words defaults to ceil(bits / 64).  Host arithmetic, no GPU.  Pass
    the block as `allow=` (2-D) with allow_bits=bits."""
    ids = np.ascontiguousarray(ids, np.uint32).ravel()
    off = np.ascontiguousarray(offsets, np.uint64).ravel()
    if off.size < 1:
        raise ValueError("offsets needs nq + 1 entries")
    nq = off.size - 1
    if int(off[-1]) > ids.size:
        raise ValueError("offsets run past the id array")
    words = (int(bits) + 63) // 64
    stride = words if stride_words is None else int(stride_words)
    out = np.empty((nq, stride), np.uint64)
    check(load().scann_hip_allow_bitmaps_from_ids(ptr(ids, u32p) if ids.size else None, ptr(off, u64p), nq, int(bits),
                                                  stride, ptr(out, u64p) if out.size else None))
    return out


def allow_bitmaps_from_ids_device(d_ids, d_offsets, nq, bits, stride_words, d_out_words, stream=0, device=0):
    """scann_hip_allow_bitmaps_from_ids_device: device addresses (integers) and a HIP stream handle; a clear and one
    scatter kernel are enqueued, nothing is synchronised.  d_out_words holds nq * stride_words uint64."""
    check(load().scann_hip_allow_bitmaps_from_ids_device(context(device), vp(d_ids), vp(d_offsets), int(nq), int(bits),
                                                         int(stride_words), vp(d_out_words), vp(stream)))


def _token_lists(token_lists):
    """(tokens uint64, offsets uint64[nq + 1]) of a list of per-query token lists"""
    lists = [np.ascontiguousarray(t, np.uint64).ravel() for t in token_lists]
    tokens = np.concatenate(lists + [np.zeros(0, np.uint64)]).astype(np.uint64)
    offsets = np.concatenate([[0], np.cumsum([t.size for t in lists])]).astype(np.uint64)
    return tokens, offsets


def _token_pairs(indices, tokens):
    idx = np.ascontiguousarray(indices, np.uint32).ravel()
    tok = np.ascontiguousarray(tokens, np.uint64).ravel()
    if idx.size != tok.size:
        raise ValueError("one token per index: %d indices, %d tokens" % (idx.size, tok.size))
    return idx, tok


class TokenMap:
    """Owns one scann_hip_token_map: RestrictTokenMap (restricts/allowlist.rs:184-244) resident on the device.  Pair i
    is add_token(indices[i], tokens[i]); indices at or past num_datapoints are ignored; the map does not change after
    it is created."""

    def __init__(self, num_datapoints, indices, tokens, device=0):
        idx, tok = _token_pairs(indices, tokens)
        self.h = vp()
        self.device = device
        check(load().scann_hip_token_map_create(context(device), int(num_datapoints), ptr(idx, u32p) if idx.size else None,
                                                ptr(tok, u64p) if tok.size else None, idx.size, C.byref(self.h)))

    def close(self):
        if self.h:
            load().scann_hip_token_map_destroy(self.h)
            self.h = None

    destroy = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_tokens(self):
        return int(load().scann_hip_token_map_num_tokens(self.h))

    def num_datapoints(self):
        return int(load().scann_hip_token_map_num_datapoints(self.h))

    def get_indices(self, token):
        """the stored posting of `token`: ascending, deduplicated, in range (the reference keeps insertion order);
        an unknown token gives an empty array"""
        n = C.c_uint64(0)
        L = load()
        status = L.scann_hip_token_map_get_indices(self.h, int(token), None, 0, C.byref(n))
        if status not in (OK, RESOURCE_EXHAUSTED):
            check(status)
        out = np.empty(n.value, np.uint32)
        if n.value:
            check(L.scann_hip_token_map_get_indices(self.h, int(token), ptr(out, u32p), out.size, C.byref(n)))
        return out

    def allow_bitmaps(self, token_lists, stride_words=None):
        """[nq, stride_words] uint64 block: row i allows the datapoints that carry at least one token of
        token_lists[i] (create_allowlist per query), built by the device kernel.  stride_words defaults to
        ceil(num_datapoints / 64).  Pass the block as `allow=` (2-D) with allow_bits=num_datapoints()."""
        tok, off = _token_lists(token_lists)
        nq = off.size - 1
        stride = (self.num_datapoints() + 63) // 64 if stride_words is None else int(stride_words)
        out = np.empty((nq, stride), np.uint64)
        check(load().scann_hip_token_map_allow_bitmaps(self.h, ptr(tok, u64p) if tok.size else None, ptr(off, u64p), nq,
                                                       stride, ptr(out, u64p) if out.size else None))
        return out

    def allow_bitmaps_device(self, d_tokens, d_offsets, nq, stride_words, d_out_words, stream=0):
        """scann_hip_token_map_allow_bitmaps_device: device addresses (integers) and a HIP stream handle; one kernel
        is enqueued, nothing is synchronised.  d_out_words holds nq * stride_words uint64."""
        check(load().scann_hip_token_map_allow_bitmaps_device(self.h, vp(d_tokens), vp(d_offsets), int(nq),
                                                              int(stride_words), vp(d_out_words), vp(stream)))

    def search_batched(self, index, queries, k, token_lists, opts=None, q_dim=None):
        """scann_hip_search_batched_tokens: query i of a tree / flat-hasher Index under the tokens of token_lists[i];
        the block is built on the device and searched on the same stream.  Returns (idx, dist, count)."""
        q = f32(queries)
        if q.ndim == 1:
            q = q[None]
        nq, qs = q.shape
        tok, off = _token_lists(token_lists)
        if off.size - 1 != nq:
            raise ValueError("one token list per query: %d lists, %d queries" % (off.size - 1, nq))
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        check(load().scann_hip_search_batched_tokens(index.h, self.h, ptr(q, f32p), nq, qs, qs if q_dim is None else q_dim,
                                                     k, C.byref(opts) if opts is not None else None,
                                                     ptr(tok, u64p) if tok.size else None, ptr(off, u64p),
                                                     ptr(out_idx, u32p), ptr(out_dist, f32p), ptr(out_cnt, u32p)))
        return out_idx, out_dist, out_cnt


def allow_bitmaps_from_tokens(indices, tokens, num_datapoints, token_lists, stride_words=None):
    """The stateless host form of TokenMap(...).allow_bitmaps(token_lists): no context, no GPU; the model the device
    forms equal bitwise."""
    idx, tok = _token_pairs(indices, tokens)
    qt, off = _token_lists(token_lists)
    nq = off.size - 1
    stride = (int(num_datapoints) + 63) // 64 if stride_words is None else int(stride_words)
    out = np.empty((nq, stride), np.uint64)
    check(load().scann_hip_allow_bitmaps_from_tokens(ptr(idx, u32p) if idx.size else None, ptr(tok, u64p) if tok.size else None,
                                                     idx.size, int(num_datapoints), ptr(qt, u64p) if qt.size else None,
                                                     ptr(off, u64p), nq, stride, ptr(out, u64p) if out.size else None))
    return out


def _attr_columns(n, columns):
    """(types int32[n_columns], the columns as contiguous arrays, a void*[n_columns] of their addresses): int64 arrays are
    ATTR_I64 columns, float32 arrays ATTR_F32 ones; anything else is refused rather than converted"""
    cols = []
    for i, c in enumerate(columns):
        c = np.asarray(c)
        if c.dtype not in (np.dtype(np.int64), np.dtype(np.float32)):
            raise ValueError("column %d: dtype %s is neither int64 nor float32" % (i, c.dtype))
        c = np.ascontiguousarray(c).ravel()
        if c.size != int(n):
            raise ValueError("column %d holds %d values, num_datapoints is %d" % (i, c.size, int(n)))
        cols.append(c)
    types = np.array([ATTR_I64 if c.dtype == np.int64 else ATTR_F32 for c in cols], np.int32)
    ptrs = (vp * max(len(cols), 1))(*[c.ctypes.data if c.size else None for c in cols])
    return types, cols, ptrs


def _range_bounds(cols_types, lo, hi):
    """[nq, n_cols, 2] uint64 bound words of a range call: cols_types[c] is clause c's type (ATTR_I64, ATTR_F32, or 0 /
    ATTR_ROW_INDEX for the row index, whose bounds are int64), lo[c] / hi[c] its per-query inclusive bounds (nq values,
    or a scalar for every query).  An f32 bound sits in the low four bytes of its word."""
    n_cols = len(cols_types)
    if len(lo) != n_cols or len(hi) != n_cols:
        raise ValueError("one lo and one hi array per clause")
    nq = max([np.size(x) for x in list(lo) + list(hi)] + [1])
    out = np.zeros((nq, n_cols, 2), np.uint64)
    for c, t in enumerate(cols_types):
        for side, x in enumerate((lo[c], hi[c])):
            if t == ATTR_F32:
                w = np.broadcast_to(np.asarray(x, np.float32), (nq,)).copy().view(np.uint32).astype(np.uint64)
            else:
                w = np.broadcast_to(np.asarray(x, np.int64), (nq,)).copy().view(np.uint64)
            out[:, c, side] = w
    return out


def _range_call(n, cols, bounds, stride, op, out):
    """(cols uint32, bounds uint64 [nq, n_cols, 2], nq, stride, the output block) of a range call's arguments"""
    cols = np.ascontiguousarray(cols, np.uint32).ravel()
    b = np.ascontiguousarray(bounds, np.uint64)
    if b.ndim != 3 or b.shape[1] != cols.size or b.shape[2] != 2:
        raise ValueError("bounds must be [nq, n_cols, 2] bound words (hip._range_bounds)")
    nq = b.shape[0]
    stride = (int(n) + 63) // 64 if stride is None else int(stride)
    if out is None:
        if op != 0:
            raise ValueError("an in-place op needs the block it combines into (out=)")
        out = np.empty((nq, stride), np.uint64)
    if out.dtype != np.uint64 or out.ndim != 2 or out.shape != (nq, stride) or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous [nq, stride] uint64 block")
    return cols, b, nq, stride, out


class AttrTable:
    """Owns one scann_hip_attr_table: typed attribute columns resident on the device.  `columns` is a list of numpy
    arrays of num_datapoints values each; int64 / float32 decide the type.  ATTR_ROW_INDEX names the row index as a
    clause column (the reference's RangeFilter).  The table does not change after it is created."""

    def __init__(self, num_datapoints, columns=(), device=0):
        types, cols, ptrs = _attr_columns(num_datapoints, columns)
        self.h = vp()
        self.device = device
        check(load().scann_hip_attr_table_create(context(device), int(num_datapoints), len(cols),
                                                 ptr(types, i32p) if len(cols) else None, ptrs, C.byref(self.h)))

    def close(self):
        if self.h:
            load().scann_hip_attr_table_destroy(self.h)
            self.h = None

    destroy = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_datapoints(self):
        return int(load().scann_hip_attr_table_num_datapoints(self.h))

    def num_columns(self):
        return int(load().scann_hip_attr_table_num_columns(self.h))

    def column_type(self, column):
        """ATTR_I64 / ATTR_F32; 0 for an unknown column"""
        return int(load().scann_hip_attr_table_column_type(self.h, int(column)))

    def clause_types(self, cols):
        """the types _range_bounds wants for the clause columns `cols` (0 for the row index)"""
        return [0 if int(c) == ATTR_ROW_INDEX else self.column_type(c) for c in cols]

    def allow_bitmaps(self, cols, bounds, stride=None, op=0, out=None):
        """[nq, stride] uint64 block: bit j of row q is the AND over the clauses of lo <= value(cols[c], j) <= hi,
        bounds = _range_bounds(...) ([nq, n_cols, 2] words), built by the device kernel.  op 0 writes a new block (or
        all of `out`); ALLOW_AND / ALLOW_OR / ALLOW_ANDNOT combine the range into `out` in place.  stride defaults to
        ceil(num_datapoints / 64).  Pass the block as `allow=` (2-D) with allow_bits=num_datapoints()."""
        cols, b, nq, stride, out = _range_call(self.num_datapoints(), cols, bounds, stride, op, out)
        check(load().scann_hip_attr_table_allow_bitmaps(self.h, ptr(cols, u32p) if cols.size else None, cols.size,
                                                        ptr(b, u64p) if b.size else None, nq, int(op), stride,
                                                        ptr(out, u64p) if out.size else None))
        return out

    def allow_bitmaps_device(self, cols, d_bounds, nq, stride_words, d_out_words, op=0, stream=0):
        """scann_hip_attr_table_allow_bitmaps_device: cols on the host, device addresses (integers) for the bound words
        and the block, a HIP stream handle; one kernel is enqueued, nothing is synchronised.  d_out_words holds nq *
        stride_words uint64."""
        cols = np.ascontiguousarray(cols, np.uint32).ravel()
        check(load().scann_hip_attr_table_allow_bitmaps_device(self.h, ptr(cols, u32p) if cols.size else None, cols.size,
                                                               vp(d_bounds or None), int(nq), int(op), int(stride_words),
                                                               vp(d_out_words), vp(stream)))

    def search_batched(self, index, queries, k, cols, bounds, opts=None, q_dim=None):
        """scann_hip_search_batched_ranges: query i of a tree / flat-hasher Index under the ranges bounds[i]; the block
        is built on the device and searched on the same stream.  Returns (idx, dist, count)."""
        q = f32(queries)
        if q.ndim == 1:
            q = q[None]
        nq, qs = q.shape
        cols = np.ascontiguousarray(cols, np.uint32).ravel()
        b = np.ascontiguousarray(bounds, np.uint64)
        if b.shape != (nq, cols.size, 2):
            raise ValueError("one range per query and clause: bounds %s, %d queries, %d clauses" % (b.shape, nq, cols.size))
        out_idx = np.full((nq, max(k, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, np.float32)
        out_cnt = np.zeros(nq, np.uint32)
        check(load().scann_hip_search_batched_ranges(index.h, self.h, ptr(q, f32p), nq, qs, qs if q_dim is None else q_dim,
                                                     k, C.byref(opts) if opts is not None else None,
                                                     ptr(cols, u32p) if cols.size else None, cols.size,
                                                     ptr(b, u64p) if b.size else None, ptr(out_idx, u32p),
                                                     ptr(out_dist, f32p), ptr(out_cnt, u32p)))
        return out_idx, out_dist, out_cnt


def search_batched_ranges(index, table, queries, k, cols, bounds, opts=None, q_dim=None):
    """scann_hip_search_batched_ranges (AttrTable.search_batched)"""
    return table.search_batched(index, queries, k, cols, bounds, opts, q_dim)


def allow_bitmaps_from_ranges(num_datapoints, columns, cols, bounds, stride=None, op=0, out=None):
    """The stateless host form of AttrTable(num_datapoints, columns).allow_bitmaps(cols, bounds, ...): no context, no
    GPU; the model the device forms equal bitwise."""
    types, arrs, ptrs = _attr_columns(num_datapoints, columns)
    cols, b, nq, stride, out = _range_call(num_datapoints, cols, bounds, stride, op, out)
    check(load().scann_hip_allow_bitmaps_from_ranges(int(num_datapoints), len(arrs), ptr(types, i32p) if len(arrs) else None,
                                                     ptrs, ptr(cols, u32p) if cols.size else None, cols.size,
                                                     ptr(b, u64p) if b.size else None, nq, int(op), stride,
                                                     ptr(out, u64p) if out.size else None))
    return out


def allow_bitmaps_combine(op, a, b, bits, out=None):
    """AndFilter / OrFilter / NotFilter over bitmap blocks on the host (scann_hip_allow_bitmaps_combine): op is
    ALLOW_AND, ALLOW_OR, ALLOW_ANDNOT (a & ~b) or ALLOW_NOT (~a, b unused).  a and b are [nq, stride] blocks or 1-D
    bitmaps shared by all queries (with no 2-D operand, nq is out's row count, else 1).  Words below ceil(bits / 64) of `out`
    (default: a zeroed [nq, ceil(bits / 64)] block) are written, the last masked to bits; its gap words are left."""
    words = (int(bits) + 63) // 64

    def operand(x):
        if x is None:
            return None, 0, None
        x = np.ascontiguousarray(x, np.uint64)
        return x, (x.shape[1] if x.ndim == 2 else 0), (x.shape[0] if x.ndim == 2 else None)

    a, sa, na = operand(a)
    b, sb, nb = operand(b)
    nq = na if na is not None else nb
    if nq is None:   # only shared operands: as many rows as `out` has, else one
        nq = out.shape[0] if out is not None and out.ndim == 2 else 1
    for x, s in ((a, sa), (b, sb)):
        if x is not None and s == 0 and x.size < words:
            raise ValueError("a shared bitmap needs ceil(bits / 64) = %d words" % words)
    if out is None:
        out = np.zeros((nq, words), np.uint64)
    if out.dtype != np.uint64 or out.ndim != 2 or out.shape[0] != nq or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous [nq, stride] uint64 block")
    check(load().scann_hip_allow_bitmaps_combine(int(op), ptr(a, u64p), sa, ptr(b, u64p), sb, nq, int(bits),
                                                 ptr(out, u64p) if out.size else None, out.shape[1]))
    return out


def allow_bitmaps_combine_device(op, d_a, stride_a, d_b, stride_b, nq, bits, d_out, stride_out, stream=0, device=0):
    """scann_hip_allow_bitmaps_combine_device: device addresses (integers; d_b = 0 for ALLOW_NOT), strides in words (0:
    one bitmap shared by all queries) and a HIP stream handle; one kernel is enqueued, nothing is synchronised.  d_out
    may be d_a or d_b with the same stride."""
    check(load().scann_hip_allow_bitmaps_combine_device(context(device), int(op), vp(d_a), int(stride_a), vp(d_b or None),
                                                        int(stride_b), int(nq), int(bits), vp(d_out), int(stride_out),
                                                        vp(stream)))


def allow_bitmap(n, allowed):
    """uint64 bitmap with bit i set for every datapoint index in `allowed`
    (restricts/allowlist.rs semantics: listed indices are allowed)."""
    bits = np.zeros((n + 63) // 64, np.uint64)
    a = np.asarray(allowed, np.uint64)
    np.bitwise_or.at(bits, (a >> np.uint64(6)).astype(np.int64), np.uint64(1) << (a & np.uint64(63)))
    return bits


def bf_create(data, n, dim, stride, measure, device=0):
    d = f32(data)
    h = vp()
    check(load().scann_hip_bf_create(context(device), ptr(d, f32p) if n else None, n, dim,
                                     stride, measure, C.byref(h)))
    return Index(h)


ROWS_BF16, ROWS_FP8_E4M3, ROWS_INT8 = 1, 2, 3
_ROWS_DTYPE = {ROWS_BF16: np.uint16, ROWS_FP8_E4M3: np.uint8, ROWS_INT8: np.int8}


def bf_create_quantized(rows, n, dim, stride, fmt, measure, inv_multiplier=1.0, device=0):
    """Brute force over rows stored as bf16 bits (uint16), the reference's E4M3 codes (uint8) or int8
    (value = i8 * inv_multiplier): scann_hip_bf_create_quantized.  The returned Index's search methods,
    bf_distances and bf_search_radius work as for bf_create."""
    dt = _ROWS_DTYPE.get(fmt, np.uint8)
    r = np.ascontiguousarray(rows).view(dt) if n else None
    if r is not None and r.size < n * stride:
        raise ValueError("rows holds %d elements, n * stride = %d" % (r.size, n * stride))
    h = vp()
    check(load().scann_hip_bf_create_quantized(context(device), r.ctypes.data if n else None, n, dim, stride, fmt,
                                               float(np.float32(inv_multiplier)), measure, C.byref(h)))
    return Index(h)


def bf16_quantize(values, device=0):
    """half::bf16::from_f32 (quantization/bfloat16.rs:13-30) on the device: uint16 bits."""
    v = f32(values)
    out = np.zeros(v.shape, np.uint16)
    check(load().scann_hip_bf16_quantize(context(device), ptr(v, f32p), v.size, ptr(out, u16p)))
    return out


def symmetric_int8(rows):
    """Host helper: symmetric per-dataset int8 codes, s = max|x| / 127, i8 = round(x / s) (half to even), and
    inv_multiplier = s.  NOT the reference's ScalarQuantizer, which writes offset-binary bytes
    (quantization/scalar.rs:162-172); bf_create_quantized reads any bytes as signed, exactly as
    ScalarQuantizedBruteForceSearcher does (brute_force/scalar_quantized.rs:198-225)."""
    x = np.asarray(rows, np.float32)
    m = float(np.max(np.abs(x))) if x.size else 0.0
    s = np.float32(m / 127.0) if m > 0 else np.float32(1.0)
    codes = np.clip(np.rint(x / s), -127, 127).astype(np.int8)
    return codes, float(s)


SQ_STDDEV, SQ_SYMMETRIC, SQ_RANGE, SQ_SIGNED = 0, 1, 2, 3   # SCANN_HIP_SQ_*


def _sq_ab(mode, num_std_devs, value_range):
    """the (a, b) arguments of the C entry points for a mode"""
    if mode == SQ_RANGE:
        if value_range is None:
            raise ValueError("SQ_RANGE needs value_range=(min, max)")
        return C.c_float(value_range[0]), C.c_float(value_range[1])
    return C.c_float(num_std_devs), C.c_float(0.0)


def _sq_params(params4, zero_point):
    return {"min": float(params4[0]), "max": float(params4[1]), "scale": float(params4[2]),
            "inv_scale": float(params4[3]), "zero_point": int(zero_point)}


def quantization_stats(index):
    """QuantizationStats::from_dataset over the f32 rows resident in `index`, on the device
    (scann_hip_index_quantization_stats): float32 [min, max, mean, std_dev]."""
    out = np.zeros(4, np.float32)
    check(load().scann_hip_index_quantization_stats(index.h, ptr(out, f32p)))
    return out


class ScalarQuantizer:
    """ScalarQuantizer (quantization/scalar.rs) through the library's stateless host functions: no GPU needed.
    mode SQ_STDDEV (the default config), SQ_SYMMETRIC, SQ_RANGE (value_range) or this library's SQ_SIGNED
    (hip.symmetric_int8 bit for bit).  calibrate(stats) takes [min, max, mean, std_dev]."""

    def __init__(self, bits=8, mode=SQ_STDDEV, num_std_devs=3.0, value_range=None):
        self.bits, self.mode = int(bits), int(mode)
        self.num_std_devs, self.value_range = num_std_devs, value_range
        self.params = np.array([0.0, 1.0, 1.0, 1.0], np.float32)   # ScalarQuantizer::new
        self.zero_point = 0

    def calibrate(self, stats):
        st = np.ascontiguousarray(stats, np.float32).ravel()
        if st.size != 4:
            raise ValueError("stats is [min, max, mean, std_dev]")
        a, b = _sq_ab(self.mode, self.num_std_devs, self.value_range)
        params = np.zeros(4, np.float32)
        zp = C.c_int32(0)
        check(load().scann_hip_scalar_quantizer_calibrate(ptr(st, f32p), self.bits, self.mode, a, b, ptr(params, f32p),
                                                          C.byref(zp)))
        self.params, self.zero_point = params, int(zp.value)
        return _sq_params(params, zp.value)

    def quantize(self, values, out=None):
        v = f32(values)
        if out is None:
            out = np.zeros(v.shape, np.int8)
        check(load().scann_hip_scalar_quantize(ptr(v, f32p) if v.size else None, v.size, self.bits, self.mode,
                                               ptr(self.params, f32p), ptr(out, i8p) if v.size else None))
        return out

    def dequantize(self, codes, out=None):
        c = np.ascontiguousarray(codes, np.int8)
        if out is None:
            out = np.zeros(c.shape, np.float32)
        check(load().scann_hip_scalar_dequantize(ptr(c, i8p) if c.size else None, c.size, self.mode,
                                                 ptr(self.params, f32p), ptr(out, f32p) if c.size else None))
        return out


def scalar_quantize_device(d_rows, n, dim, stride, d_out, out_stride, params4, bits=8, mode=SQ_STDDEV, stream=0, device=0):
    """scann_hip_scalar_quantize_device: device addresses (integers) and a HIP stream handle; one kernel is enqueued,
    nothing is synchronised.  d_out holds n * out_stride int8; params4 = [min, max, scale, inv_scale]."""
    p = np.ascontiguousarray(params4, np.float32).ravel()
    check(load().scann_hip_scalar_quantize_device(context(device), vp(d_rows), int(n), int(dim), int(stride), int(bits),
                                                  int(mode), ptr(p, f32p), vp(d_out), int(out_stride), vp(stream or None)))


def txh_create(*, data, n_rows, dim, stride, centers, leaf_offsets, leaf_ids, codebook, codes,
               codes_packed4=False, use_residuals=True, partitions_to_search=10,
               pre_reorder_multiplier=3.0, leaf_sizes_global=None, data_is_csr_order=False,
               distance_measure=SQUARED_L2, device=0):
    """codebook=None and codes=None: SearchMode::Partitioned (exact scan of the selected leaves)."""
    d, keep = _txh_desc(data=data, n_rows=n_rows, dim=dim, stride=stride, centers=centers,
                        leaf_offsets=leaf_offsets, leaf_ids=leaf_ids, codebook=codebook, codes=codes,
                        codes_packed4=codes_packed4, use_residuals=use_residuals,
                        partitions_to_search=partitions_to_search,
                        pre_reorder_multiplier=pre_reorder_multiplier, leaf_sizes_global=leaf_sizes_global,
                        data_is_csr_order=data_is_csr_order, distance_measure=distance_measure)
    h = vp()
    check(load().scann_hip_txh_create(context(device), C.byref(d), C.byref(h)))
    return Index(h)


def txh_create_quantized(*, rows, fmt, inv_multiplier=1.0, device=0, **desc):
    """A tree / hasher index whose re-rank rows are stored as bf16 bits (uint16), the reference's E4M3 codes (uint8) or
    int8 (value = i8 * inv_multiplier): scann_hip_txh_create_quantized.  `rows` [n_rows, stride] elements, indexed as
    txh_create's data; `desc`: txh_create's keyword arguments without data."""
    if desc.get("data") is not None:
        raise ValueError("txh_create_quantized takes rows=, not data=")
    desc["data"] = None
    d, keep = _txh_desc(**desc)
    r = None if rows is None else np.ascontiguousarray(rows).view(_ROWS_DTYPE.get(fmt, np.uint8))
    if r is not None and r.size < d.n_rows * d.stride:
        raise ValueError("rows holds %d elements, n_rows * stride = %d" % (r.size, d.n_rows * d.stride))
    h = vp()
    check(load().scann_hip_txh_create_quantized(context(device), C.byref(d), r.ctypes.data if r is not None else None,
                                                fmt, float(np.float32(inv_multiplier)), C.byref(h)))
    return Index(h)


PROJ_MATRIX, PROJ_PCA, PROJ_TRUNCATE = 1, 2, 3   # SCANN_HIP_PROJ_*


class Projection:
    """Owns one scann_hip_projection: the reference's dense projections (out[j] = sum over ascending i of
    (in[i] - mean[i]) * matrix[j, i], f32, a multiply then an add per step; the mean PCA's alone) and TruncateProjection
    (out = in[start : start + out_dim]).  `matrix` is [out_dim, in_dim]; immutable after create."""

    def __init__(self, kind, matrix=None, mean=None, in_dim=None, out_dim=None, start=0, device=0):
        m = None if matrix is None else f32(matrix)
        mu = None if mean is None else f32(mean).ravel()
        if m is not None and m.ndim == 2:
            out_dim = m.shape[0] if out_dim is None else out_dim
            in_dim = m.shape[1] if in_dim is None else in_dim
            if m.shape != (out_dim, in_dim):
                raise ValueError("matrix is %s, not [out_dim, in_dim] = [%d, %d]" % (m.shape, out_dim, in_dim))
        if mu is not None and in_dim is not None and mu.size != in_dim:
            raise ValueError("mean holds %d values, in_dim = %d" % (mu.size, in_dim))
        h = vp()
        check(load().scann_hip_projection_create(context(device), int(kind), int(in_dim or 0), int(out_dim or 0),
                                                 ptr(m, f32p), ptr(mu, f32p), int(start), C.byref(h)))
        self.h = h

    @classmethod
    def from_handle(cls, h):
        """Owns a scann_hip_projection the library made (pca_train)."""
        p = cls.__new__(cls)
        p.h = h
        return p

    def arrays(self):
        """(matrix [out_dim, in_dim] or None for TRUNCATE, mean [in_dim] or None unless PCA): scann_hip_projection_arrays"""
        kind, in_dim, out_dim, _ = self.info()
        m = np.zeros((out_dim, in_dim), np.float32) if kind != PROJ_TRUNCATE else None
        mu = np.zeros(in_dim, np.float32) if kind == PROJ_PCA else None
        check(load().scann_hip_projection_arrays(self.h, ptr(m, f32p), ptr(mu, f32p)))
        return m, mu

    def close(self):
        if getattr(self, "h", None):
            load().scann_hip_projection_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """(kind, in_dim, out_dim, start)"""
        out = np.zeros(4, np.uint32)
        check(load().scann_hip_projection_info(self.h, ptr(out, u32p)))
        return tuple(int(v) for v in out)

    def project(self, rows, row_dim=None, out=None):
        """rows [n, row_stride] (row_dim leading columns are the row; default all) -> [n, out_dim], or into `out`
        [n, out_stride], whose columns past out_dim are left as they are (scann_hip_project)."""
        r = f32(rows)
        if r.ndim == 1:
            r = r[None]
        n, rs = r.shape
        od = self.info()[2]
        o = np.empty((n, od), np.float32) if out is None else out
        if o.dtype != np.float32 or not o.flags.c_contiguous or o.ndim != 2 or o.shape[0] != n:
            raise ValueError("out must be a C-contiguous float32 [n, out_stride] array")
        check(load().scann_hip_project(self.h, ptr(r, f32p) if n else None, n, rs, rs if row_dim is None else row_dim,
                                       ptr(o, f32p) if n else None, o.shape[1]))
        return o

    def project_device(self, d_rows, n, row_stride, d_out, out_stride, stream=0):
        """scann_hip_project_device: device addresses (integers) and a HIP stream handle; one kernel is enqueued, nothing is
        synchronised or allocated."""
        check(load().scann_hip_project_device(self.h, vp(d_rows), int(n), int(row_stride), vp(d_out), int(out_stride),
                                              vp(stream or None)))


def txh_create_projected(*, projection, rows, row_dim, row_stride=None, n_rows=None, device=0, **desc):
    """A tree / hasher index that partitions, hashes and scans in the projected space and re-ranks against the original
    `rows` [n_rows, row_stride] (None: no exact re-ordering): scann_hip_txh_create_projected.  `desc`: txh_create's
    keyword arguments for the index in the projected space, without data / n_rows / stride (dim = the projection's
    out_dim).  Searches take queries of row_dim floats."""
    if desc.get("data") is not None:
        raise ValueError("txh_create_projected takes rows=, not data=")
    r = None if rows is None else f32(rows)
    if r is not None and r.ndim == 2:
        row_stride = r.shape[1] if row_stride is None else row_stride
        n_rows = r.shape[0] if n_rows is None else n_rows
    row_stride = row_dim if row_stride is None else row_stride
    n_rows = 0 if n_rows is None else n_rows
    if r is not None and r.size < n_rows * row_stride:
        raise ValueError("rows holds %d elements, n_rows * row_stride = %d" % (r.size, n_rows * row_stride))
    desc["data"] = None
    desc.setdefault("stride", desc.get("dim"))
    desc["n_rows"] = n_rows
    d, keep = _txh_desc(**desc)
    h = vp()
    check(load().scann_hip_txh_create_projected(context(device), C.byref(d), projection.h if projection is not None else None,
                                                ptr(r, f32p), int(n_rows), int(row_dim), int(row_stride), C.byref(h)))
    return Index(h)


def txh_write_file(path, *, device=None, **kw):
    """Write the index the same keyword arguments would create (no GPU needed)."""
    d, keep = _txh_desc(**kw)
    check(load().scann_hip_txh_write_file(os.fsencode(path), C.byref(d)))


def bf_write_file(path, data, n, dim, stride, measure):
    d = f32(data)
    check(load().scann_hip_bf_write_file(os.fsencode(path), ptr(d, f32p) if n else None, n, dim, stride, measure))


def index_file_info(path):
    info = FileInfo()
    check(load().scann_hip_index_file_info(os.fsencode(path), C.byref(info)))
    return {name: getattr(info, name) for name, _ in FileInfo._fields_}


def index_write_file(index, path):
    """Write a handle's arrays, read back from the device, to the index container (scann_hip_index_write_file)."""
    check(load().scann_hip_index_write_file(index.h, os.fsencode(path)))


def load_file(path, device=0):
    """mmap the index file and upload it (scann_hip_index_load_file)."""
    h = vp()
    check(load().scann_hip_index_load_file(context(device), os.fsencode(path), C.byref(h)))
    return Index(h)


def _txh_desc(*, data, n_rows, dim, stride, centers, leaf_offsets, leaf_ids, codebook, codes,
              codes_packed4=False, use_residuals=True, partitions_to_search=10,
              pre_reorder_multiplier=3.0, leaf_sizes_global=None, data_is_csr_order=False,
              distance_measure=SQUARED_L2):
    d = TxhDesc()
    keep = []

    def hold(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a

    data = hold(data, np.float32)
    centers = hold(centers, np.float32)
    leaf_offsets = hold(leaf_offsets, np.uint32)
    leaf_ids = hold(leaf_ids, np.uint32)
    leaf_sizes_global = hold(leaf_sizes_global, np.uint32)
    codebook = hold(codebook, np.float32)
    codes = hold(codes, np.uint8)
    d.data = ptr(data, f32p)
    d.n_rows = n_rows
    d.dim = dim
    d.stride = stride
    d.data_is_csr_order = 1 if data_is_csr_order else 0
    d.centers = ptr(centers, f32p)
    d.num_partitions = 0 if centers is None else centers.shape[0]
    d.leaf_offsets = ptr(leaf_offsets, u32p)
    d.leaf_ids = ptr(leaf_ids, u32p)
    d.leaf_sizes_global = ptr(leaf_sizes_global, u32p)
    d.n_local = codes.shape[0] if codes is not None else leaf_ids.shape[0]
    d.codebook = ptr(codebook, f32p)
    if codebook is not None:
        d.num_subspaces, d.num_codes, d.dims_per_subspace = codebook.shape
    d.codes = ptr(codes, u8p)
    d.distance_measure = distance_measure
    d.codes_packed4 = 1 if codes_packed4 else 0
    d.use_residuals = 1 if use_residuals else 0
    d.partitions_to_search = partitions_to_search
    d.pre_reorder_multiplier = pre_reorder_multiplier
    return d, keep


def txh_partition(index, queries, num_partitions, q_dim=None):
    q = f32(queries)
    nq, qs = q.shape
    tok = np.zeros((nq, max(num_partitions, 1)), np.uint32)
    dist = np.zeros((nq, max(num_partitions, 1)), np.float32)
    cnt = np.zeros(nq, np.uint32)
    check(load().scann_hip_txh_partition(index.h, ptr(q, f32p), nq, qs, qs if q_dim is None else q_dim,
                                         num_partitions, ptr(tok, u32p), ptr(dist, f32p),
                                         ptr(cnt, u32p)))
    return tok, dist, cnt


def lut_from_query(index, queries, S, K, leaf_for_query=None):
    q = f32(queries)
    nq, qs = q.shape
    out = np.zeros((nq, S, K), np.float32)
    lf = None if leaf_for_query is None else np.ascontiguousarray(leaf_for_query, np.uint32)
    check(load().scann_hip_lut_from_query(index.h, ptr(q, f32p), nq, qs, ptr(lf, u32p),
                                          ptr(out, f32p)))
    return out


def adc_distances(index, luts):
    luts = f32(luts)
    nq = luts.shape[0]
    out = np.zeros((nq, index.size()), np.float32)
    check(load().scann_hip_adc_distances(index.h, ptr(luts, f32p), nq, ptr(out, f32p)))
    return out


def lut16_distances_batch(packed, lut8, S, n, bias, mult, device=0):
    packed = np.ascontiguousarray(packed, np.uint8)
    lut8 = np.ascontiguousarray(lut8, np.uint8)
    out = np.zeros(n, np.float32)
    check(load().scann_hip_lut16_distances_batch(context(device), ptr(packed, u8p), ptr(lut8, u8p),
                                                 S, n, bias, mult, ptr(out, f32p)))
    return out


def lut16_quantize(tables, device=0):
    """Lut16SimdTables::from_float_tables on the device: (lut8 [S][16] u8, bias, multiplier)."""
    t = f32(tables)
    S = t.shape[0]
    lut8 = np.zeros((S, 16), np.uint8)
    bias = C.c_float(0)
    mult = C.c_float(0)
    check(load().scann_hip_lut16_quantize(context(device), ptr(t, f32p) if S else None, S,
                                          ptr(lut8, u8p) if S else None, C.byref(bias), C.byref(mult)))
    return lut8, float(np.float32(bias.value)), float(np.float32(mult.value))


FP8_E4M3, FP8_E5M2 = 0, 1


def fp8_quantize(values, scale=1.0, fmt=FP8_E4M3, device=0):
    """Quantizer::quantize over Fp8Quantizer (quantization/fp8.rs:247-255) on the device."""
    v = f32(values)
    out = np.zeros(v.shape, np.uint8)
    check(load().scann_hip_fp8_quantize(context(device), ptr(v, f32p), v.size, float(np.float32(scale)), fmt,
                                        ptr(out, u8p)))
    return out


def fp8_dequantize(bits, scale=1.0, fmt=FP8_E4M3, device=0):
    b = np.ascontiguousarray(bits, np.uint8)
    out = np.zeros(b.shape, np.float32)
    check(load().scann_hip_fp8_dequantize(context(device), ptr(b, u8p), b.size, float(np.float32(scale)), fmt,
                                          ptr(out, f32p)))
    return out


def fp8_distances(query, database, stride, n, measure, device=0):
    """one_to_many_fp8_float_{squared_l2,dot_product} (one_to_many_asymmetric.rs:327-377)."""
    q = f32(query)
    db = np.ascontiguousarray(database, np.uint8)
    out = np.zeros(n, np.float32)
    check(load().scann_hip_fp8_distances(context(device), ptr(q, f32p), q.size, ptr(db, u8p), stride, n, measure,
                                         ptr(out, f32p)))
    return out


def abi_layout(words=6):
    """The first `words` layout words of scann_hip_abi_layout: 6 = the descriptor, search options and file info;
    10 adds sizeof / last-field offset of scann_hip_build_config and scann_hip_build_report."""
    out = np.zeros(words, np.uint32)
    n = load().scann_hip_abi_layout(ptr(out, u32p), words)
    return [int(v) for v in out[:n]]


_LAYOUT_KEYS = ["qr", "nq_pad", "block_bytes", "blk_idx", "blk_exact", "blk_count", "soa_bytes", "soa_idx",
                "soa_exact", "soa_count", "res_bytes", "res_dist", "blk_keys", "cap", "blk_flag", "res_status"]


def comm_layout(nq, world, m_local, k):
    """scann_hip_comm_layout as a dict (no GPU needed)."""
    out = np.zeros(16, np.uint64)
    check(load().scann_hip_comm_layout(nq, world, m_local, k, ptr(out, u64p)))
    return {n: int(v) for n, v in zip(_LAYOUT_KEYS, out)}


class Comm:
    """One RCCL communicator of the library (scann_hip_comm_*)."""

    def __init__(self, unique_id, rank, world, device=0):
        h = vp()
        self._id = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        check(load().scann_hip_comm_create(context(device), C.cast(self._id, vp), rank, world, C.byref(h)))
        self.h, self.rank, self.world = h, rank, world

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        check(load().scann_hip_comm_unique_id(C.cast(buf, vp)))
        return bytes(buf)

    def last_status(self):
        check(load().scann_hip_comm_last_status(self.h))

    def close(self):
        if self.h:
            load().scann_hip_comm_destroy(self.h)
            self.h = None


def encode(codebook, rows, stride=None, centers=None, leaf_of_row=None, device=0):
    cb = f32(codebook)
    rows = f32(rows)
    n = rows.shape[0]
    st = rows.shape[1] if stride is None else stride
    S, K, dsub = cb.shape
    out = np.zeros((n, S), np.uint8)
    cen = None if centers is None else f32(centers)
    lf = None if leaf_of_row is None else np.ascontiguousarray(leaf_of_row, np.uint32)
    check(load().scann_hip_encode(context(device), ptr(cb, f32p), S, K, dsub, ptr(rows, f32p), n,
                                  st, ptr(cen, f32p), ptr(lf, u32p), ptr(out, u8p)))
    return out


def bf_distances(index, queries):
    q = f32(queries)
    nq, qs = q.shape
    out = np.zeros((nq, index.size()), np.float32)
    check(load().scann_hip_bf_distances(index.h, ptr(q, f32p), nq, qs, ptr(out, f32p)))
    return out


def bf_search_radius(index, query, radius, capacity=None, allow=None, allow_bits=None):
    """BruteForceSearcher::search_radius: (idx, dist) of every row with distance <= radius.  `allow`, `allow_bits`:
    an allow-bitmap and its capacity as in Index.search_batched -- only allowed rows are returned."""
    q = f32(query).reshape(-1)
    cap = index.size() if capacity is None else int(capacity)
    idx = np.zeros(max(cap, 1), np.uint32)
    dist = np.zeros(max(cap, 1), np.float32)
    cnt = C.c_uint64(0)
    if allow is not None:
        allow = np.ascontiguousarray(allow, np.uint64)
        o = default_opts()
        o.allow_bitmap, o.allow_bitmap_bits = ptr(allow, u64p), _allow_capacity(allow, allow_bits)
        check(load().scann_hip_bf_search_radius_opts(index.h, ptr(q, f32p), q.size, C.c_float(radius), C.byref(o),
                                                     ptr(idx, u32p), ptr(dist, f32p), C.c_uint64(cap), C.byref(cnt)))
    else:
        check(load().scann_hip_bf_search_radius(index.h, ptr(q, f32p), q.size, C.c_float(radius),
                                                ptr(idx, u32p), ptr(dist, f32p), C.c_uint64(cap),
                                                C.byref(cnt)))
    n = min(int(cnt.value), cap)
    return idx[:n], dist[:n], int(cnt.value)


KMEANS_SIMD_THRESHOLD = 128   # KMeansConfig::default().simd_threshold (trees/kmeans.rs:59)


def kmeans_init_pp(index, k, seed, col_offset=0, sub_dim=None, simd_threshold=KMEANS_SIMD_THRESHOLD):
    """k-means++ seeding on the GPU over the rows of a brute-force index: centres [k][sub_dim]."""
    sd = index.dimensionality() if sub_dim is None else sub_dim
    out = np.zeros((k, sd), np.float32)
    check(load().scann_hip_kmeans_init_pp(index.h, col_offset, sd, k, C.c_uint64(seed), simd_threshold,
                                          ptr(out, f32p)))
    return out


def kmeans_lloyd(index, centers, max_iterations=100, convergence_threshold=1e-5, col_offset=0,
                 simd_threshold=KMEANS_SIMD_THRESHOLD):
    """KMeans::fit_single's Lloyd loop on the GPU from given centres.
    Returns (centers, assign, sizes, inertia, iterations, converged)."""
    c = np.array(centers, np.float32, copy=True, order="C")
    k, sd = c.shape
    n = index.size()
    assign = np.zeros(n, np.uint32); sizes = np.zeros(k, np.uint32)
    inertia = C.c_double(0); iters = C.c_uint32(0); conv = C.c_int(0)
    check(load().scann_hip_kmeans_lloyd(index.h, col_offset, sd, ptr(c, f32p), k, max_iterations,
                                        C.c_double(convergence_threshold), simd_threshold, ptr(assign, u32p),
                                        ptr(sizes, u32p), C.byref(inertia),
                                        C.cast(C.byref(iters), u32p), C.byref(conv)))
    return c, assign, sizes, inertia.value, iters.value, bool(conv.value)


BUILD_STAGES = ("partition_seeding", "partition_lloyd", "csr_residuals", "codebook_seeding", "codebook_lloyd",
                "encode", "finish")


def build_config(**cfg):
    """scann_hip_build_config_default with the keyword arguments set on top (field names of BuildConfig)."""
    c = BuildConfig()
    load().scann_hip_build_config_default(C.byref(c))
    names = {f for f, _ in BuildConfig._fields_}
    for key, value in cfg.items():
        if key not in names:
            raise TypeError("scann_hip_build_config has no field %r" % key)
        setattr(c, key, value)
    return c


def txh_build(bf_index, **cfg):
    """scann_hip_txh_build: a tree (num_partitions > 0) or flat-hasher (0) index trained, encoded and laid out on the
    device from the resident rows of an f32 brute-force index.  Returns (Index, report): report is a dict with
    partition_iterations / _converged / _inertia, subspace_iterations and subspace_converged ([S] lists) and stage_ms
    ({stage name: milliseconds}, BUILD_STAGES)."""
    c = build_config(**cfg)
    rep = BuildReport()
    h = vp()
    check(load().scann_hip_txh_build(bf_index.h, C.byref(c), C.byref(h), C.byref(rep)))
    return Index(h), _build_report(rep, c.num_subspaces)


def _build_report(rep, S):
    return dict(partition_iterations=int(rep.partition_iterations), partition_converged=bool(rep.partition_converged),
                partition_inertia=float(rep.partition_inertia),
                subspace_iterations=[int(v) for v in rep.subspace_iterations[:S]],
                subspace_converged=[bool(v) for v in rep.subspace_converged[:S]],
                stage_ms=dict(zip(BUILD_STAGES, (float(v) for v in rep.stage_ms))))


def tree_config(**kw):
    """scann_hip_tree_config_default with the keyword arguments set on top (field names of TreeConfig)."""
    c = TreeConfig()
    load().scann_hip_tree_config_default(C.byref(c))
    names = {f for f, _ in TreeConfig._fields_}
    for key, value in kw.items():
        if key not in names:
            raise TypeError("scann_hip_tree_config has no field %r" % key)
        setattr(c, key, value)
    return c


def txh_build_hierarchical(bf_index, tree=None, **cfg):
    """scann_hip_txh_build_hierarchical: txh_build with the partitioner of TreePartitioner::build_hierarchical -- a k-means
    tree trained level by level on the device and flattened to its leaves.  `tree`: a TreeConfig, a dict of its fields, or
    None for the defaults; of **cfg, num_partitions and the kmeans_* fields are ignored.  Returns (Index, report,
    tree_report): report as txh_build's (the partition_* slots hold the root's k-means), tree_report a dict with
    num_leaves, depth_reached, the per-level lists level_nodes / level_iterations / level_converged / level_leaves
    (depths 0..4) and stage_ms ([(seeding, lloyd)] per level, milliseconds)."""
    t = tree if isinstance(tree, TreeConfig) else tree_config(**(tree or {}))
    c = build_config(**cfg)
    rep, trep = BuildReport(), TreeReport()
    h = vp()
    check(load().scann_hip_txh_build_hierarchical(bf_index.h, C.byref(t), C.byref(c), C.byref(h), C.byref(rep),
                                                  C.byref(trep)))
    tree_report = dict(num_leaves=int(trep.num_leaves), depth_reached=int(trep.depth_reached),
                       level_nodes=[int(v) for v in trep.level_nodes],
                       level_iterations=[int(v) for v in trep.level_iterations],
                       level_converged=[int(v) for v in trep.level_converged],
                       level_leaves=[int(v) for v in trep.level_leaves],
                       stage_ms=[(float(trep.stage_ms[2 * d]), float(trep.stage_ms[2 * d + 1])) for d in range(5)])
    return Index(h), _build_report(rep, c.num_subspaces), tree_report


def txh_build_projected(bf_index, projection, **cfg):
    """scann_hip_txh_build_projected: txh_build of a PROJECTED index in one call -- the rows of the f32 brute-force index
    (projection.in_dim floats each) are projected on the device, the tree / flat hasher is trained, encoded and laid out
    in the projected space, and the handle re-ranks against the original rows (store_rows=1) or holds none.  Returns
    (Index, report) as txh_build does; stage_ms["partition_seeding"] includes the projection pass."""
    c = build_config(**cfg)
    rep = BuildReport()
    h = vp()
    check(load().scann_hip_txh_build_projected(bf_index.h, projection.h if projection is not None else None, C.byref(c),
                                               C.byref(h), C.byref(rep)))
    return Index(h), _build_report(rep, c.num_subspaces)


PCA_STAGES = ("sample_mean", "covariance", "eigen_solve", "components")


def pca_train(bf_index, out_dim, max_samples=0, seed=42, want_eigenvalues=False, want_covariance=False):
    """scann_hip_pca_train: a PROJ_PCA Projection trained on the device from the rows of an f32 brute-force index (the rule
    of trainer.pca_projection; max_samples 0 = every row).  Returns (projection, info): info holds sweeps, converged,
    and, when asked for, eigenvalues (f64 [in_dim], descending) and covariance (f64 [in_dim, in_dim])."""
    d = bf_index.dimensionality()
    eig = np.zeros(d, np.float64) if want_eigenvalues else None
    cov = np.zeros((d, d), np.float64) if want_covariance else None
    sweeps, conv, h = C.c_uint32(0), C.c_int(0), vp()
    f64p = C.POINTER(C.c_double)
    check(load().scann_hip_pca_train(bf_index.h, int(out_dim), int(max_samples), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h),
                                     ptr(eig, f64p), ptr(cov, f64p), C.cast(C.byref(sweeps), u32p), C.byref(conv)))
    info = dict(sweeps=int(sweeps.value), converged=bool(conv.value))
    if want_eigenvalues:
        info["eigenvalues"] = eig
    if want_covariance:
        info["covariance"] = cov
    return Projection.from_handle(h), info


def pca_last_stage_ms():
    """{stage: host-clock milliseconds} of this thread's last pca_train (PCA_STAGES)"""
    out = np.zeros(4, np.float32)
    load().scann_hip_pca_last_stage_ms(ptr(out, f32p))
    return dict(zip(PCA_STAGES, (float(v) for v in out)))


def bf_assign_nearest(index, centers, want_dist=True):
    c = f32(centers)
    n = index.size()
    out = np.zeros(n, np.uint32)
    dist = np.zeros(n, np.float32) if want_dist else None
    check(load().scann_hip_bf_assign_nearest(index.h, ptr(c, f32p), c.shape[0], ptr(out, u32p),
                                             ptr(dist, f32p)))
    return (out, dist) if want_dist else out


def assign_leaves(sizes, world):
    sizes = np.ascontiguousarray(sizes, np.uint32)
    owner = np.zeros(sizes.size, np.uint32)
    check(load().scann_hip_assign_leaves(ptr(sizes, u32p), sizes.size, world, ptr(owner, u32p)))
    return owner
