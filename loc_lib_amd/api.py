"""ctypes binding of ``liblocgpu.so`` (the C ABI in ``include/locgpu.h``).

This is test/bench plumbing around the product library: every call goes straight through the C ABI to the
HIP kernels. There is no CPU fallback — if the library or a GPU is missing the calls raise ``LocGpuError``.
Class and method names mirror the reference's matcher interface
(``LocUtils::IcpRegistration`` / ``NdtRegistration``: SetInputTarget, ScanMatch, CaculateMatrixHAndB —
LocUtils/include/LocUtils/model/matching/3d/matching_interface.h:13-54).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOCGPU_LIB") or os.path.join(_HERE, "liblocgpu.so")  # LOCGPU_LIB: A/B builds of the same library
CSRC = os.path.join(_HERE, "csrc")

P2P, P2LINE, P2PLANE = 0, 1, 2
P2PLANE_MAP = 5  # labelled fast mode: planes fitted once per map point at ingest; never a parity source
SEARCH_TREE_FAITHFUL, SEARCH_GRID_EXACT = 0, 1
CENTER, NEARBY6 = 0, 1
DIRECT_NDT, INCREMENTAL_NDT = 1, 2
# The `method` of the Gauss–Newton solve stage for the two NDT variants (csrc/icp_kernels.hpp: kMethodNdtDirect, kMethodNdtInc — the
# values locgpu_icp_method leaves free); Context.debug_gn_solve takes them beside P2P, P2LINE, P2PLANE and P2PLANE_MAP.
SOLVE_NDT_DIRECT, SOLVE_NDT_INC = 3, 4
ACC_W, HB_W, LOAM_HB_W = 32, 44, 46  # doubles per block partial (21 H, 6 B, effective_num, 4 spare) / per hb row of the solve / of the LOAM solve
# One row of state_in / state_out of the solve-stage test hooks: the library's per-scan state, 160 bytes (include/locgpu.h).
SOLVE_STATE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("R", "<f8", (9,)), ("last_dx_norm", "<f8"), ("last_eff", "<i8"),
                        ("iterations", "<i4"), ("converged", "<i4"), ("done", "<i4"), ("status", "<i4")])
assert SOLVE_STATE.itemsize == 160

# every symbol include/locgpu.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "locgpu_icp_opts_default", "locgpu_ndt_opts_default", "locgpu_create", "locgpu_destroy", "locgpu_last_error",
    "locgpu_device_count", "locgpu_icp_set_target", "locgpu_icp_set_target_async", "locgpu_icp_target_info", "locgpu_knn", "locgpu_icp_hb", "locgpu_icp_align",
    "locgpu_transform_cloud", "locgpu_batch_create", "locgpu_batch_destroy", "locgpu_icp_align_batch", "locgpu_ndt_align_batch",
    "locgpu_icp_hb_batch", "locgpu_gn_update", "locgpu_ndt_set_target", "locgpu_ndt_target_info", "locgpu_ndt_dump", "locgpu_debug_ndt_slots",
    "locgpu_ndt_align", "locgpu_profile_enable", "locgpu_profile_read", "locgpu_visit_count_enable", "locgpu_visit_count_read",
    "locgpu_search_stats_read", "locgpu_debug_batch_nn", "locgpu_debug_batch_run_flags", "locgpu_debug_batch_slot", "locgpu_graph_enable",
    "locgpu_debug_gn_solve", "locgpu_debug_loam_solve",
    "locgpu_cloud_create", "locgpu_cloud_destroy", "locgpu_cloud_upload", "locgpu_cloud_info", "locgpu_cloud_download", "locgpu_cloud_copy",
    "locgpu_cloud_remove_nan", "locgpu_cloud_voxel_filter", "locgpu_cloud_crop_box", "locgpu_cloud_transform", "locgpu_cloud_append",
    "locgpu_icp_set_target_cloud", "locgpu_icp_set_target_cloud_async", "locgpu_ndt_set_target_cloud", "locgpu_icp_align_cloud", "locgpu_ndt_align_cloud",
    "locgpu_voxel_filter", "locgpu_crop_box", "locgpu_remove_nan",
    "locgpu_submap_create", "locgpu_submap_destroy", "locgpu_submap_add_keyframe", "locgpu_submap_cloud", "locgpu_submap_last_keyframe",
    "locgpu_submap_info", "locgpu_cloud_loam_extract", "locgpu_loam_extract",
    "locgpu_batch_create_empty", "locgpu_batch_upload_async", "locgpu_batch_upload_wait",
    "locgpu_bfnn_set_target", "locgpu_bfnn_knn",
    "locgpu_icp_align_batch_begin", "locgpu_ndt_align_batch_begin", "locgpu_align_batch_end",
    "locgpu_comm_unique_id", "locgpu_comm_init", "locgpu_comm_info", "locgpu_batch_create_sharded", "locgpu_icp_set_target_bcast",
    "locgpu_pool_opts_default", "locgpu_pool_create", "locgpu_pool_destroy", "locgpu_pool_submit", "locgpu_pool_wait", "locgpu_pool_info",
    "locgpu_pool_profile_read", "locgpu_pool_step", "locgpu_pool_done",
    "locgpu_icp_scan_match", "locgpu_ndt_scan_match",
    "locgpu_icp_fitness", "locgpu_icp_fitness_batch", "locgpu_icp_fitness_resident", "locgpu_batch_create_shared",
    "locgpu_init_search_opts_default", "locgpu_icp_init_search", "locgpu_pose_grid",
    "locgpu_ndt_fitness", "locgpu_ndt_fitness_batch", "locgpu_ndt_fitness_resident", "locgpu_ndt_init_search", "locgpu_ndt_hb", "locgpu_ndt_hb_batch",
    "locgpu_icp_build_map_planes", "locgpu_icp_map_planes_info", "locgpu_icp_map_planes_dump",
    "locgpu_loam_opts_default", "locgpu_loam_create", "locgpu_loam_destroy", "locgpu_loam_last_error", "locgpu_loam_set_target",
    "locgpu_loam_hb", "locgpu_loam_scan_match", "locgpu_loam_align_batch",
    "locgpu_loam_set_target_cloud", "locgpu_loam_set_target_cloud_async", "locgpu_loam_scan_match_cloud", "locgpu_loam_fitness_resident",
    "locgpu_loam_submap_create", "locgpu_loam_submap_destroy", "locgpu_loam_submap_add_keyframe", "locgpu_loam_submap_clouds", "locgpu_loam_submap_info",
    "locgpu_loam_create_on", "locgpu_loam_fitness", "locgpu_loam_fitness_cloud", "locgpu_loam_init_search", "locgpu_loam_init_search_cloud",
    "locgpu_batch_preprocess", "locgpu_batch_upload_clouds", "locgpu_batch_download_scan",
    "locgpu_batch_loam_extract", "locgpu_loam_align_batches",
    "locgpu_clouds_merge", "locgpu_batch_merge", "locgpu_batch_export_cloud",
    "locgpu_sensor_create", "locgpu_sensor_destroy", "locgpu_batch_upload_ranges", "locgpu_batch_download_rings",
    "locgpu_batch_loam_extract_resident", "locgpu_cloud_upload_ranges", "locgpu_range_ingest_times",
    "locgpu_sensor_set_col_times", "locgpu_batch_upload_ranges_deskew", "locgpu_cloud_upload_ranges_deskew", "locgpu_range_deskew_matrices",
    "locgpu_range_deskew_times",
    "locgpu_batch_upload_records", "locgpu_batch_upload_records_deskew", "locgpu_cloud_upload_records", "locgpu_cloud_upload_records_deskew",
    "locgpu_records_deskew_debug", "locgpu_records_deskew_matrices", "locgpu_records_ingest_times",
    "locgpu_batch_keep_times", "locgpu_batch_download_times", "locgpu_batch_deskew", "locgpu_batch_deskew_times", "locgpu_motion_from_poses",
    "locgpu_icp_set_target_forest", "locgpu_icp_set_target_forest_batch", "locgpu_icp_forest_info", "locgpu_icp_align_pairs", "locgpu_icp_fitness_pairs",
    "locgpu_ndt_set_target_set", "locgpu_ndt_set_target_set_batch", "locgpu_ndt_set_info", "locgpu_ndt_set_dump", "locgpu_ndt_align_pairs", "locgpu_ndt_fitness_pairs",
    "locgpu_icp_set_target_forest_device", "locgpu_icp_set_target_cloud_device", "locgpu_icp_device_build_info", "locgpu_debug_tree_read",
]
BUILD_PATH_NONE, BUILD_PATH_DEVICE, BUILD_PATH_HOST = 0, 1, 2  # locgpu_icp_device_build_info: out[0]
STATUS_NO_PAIR_TARGET = 5  # LOCGPU_STATUS_NO_PAIR_TARGET
COMM_ID_BYTES = 128
NO_INTENSITY = ctypes.c_size_t(-1).value


class LocGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("locgpu error %d: %s" % (code, msg))
        self.code = code


class IcpOpts(ctypes.Structure):
    _fields_ = [("method", ctypes.c_int32), ("max_iteration", ctypes.c_int32), ("max_nn_distance", ctypes.c_double),
                ("max_plane_distance", ctypes.c_double), ("max_line_distance", ctypes.c_double), ("min_effective_pts", ctypes.c_int32),
                ("eps", ctypes.c_double), ("approximate", ctypes.c_int32), ("ann_alpha", ctypes.c_float), ("search_mode", ctypes.c_int32)]


class NdtOpts(ctypes.Structure):
    _fields_ = [("max_iteration", ctypes.c_int32), ("voxel_size", ctypes.c_double), ("min_effective_pts", ctypes.c_int32),
                ("min_pts_in_voxel", ctypes.c_int32), ("eps", ctypes.c_double), ("res_outlier_th", ctypes.c_double),
                ("nearby_type", ctypes.c_int32), ("method", ctypes.c_int32), ("capacity", ctypes.c_int64)]


class LoamOpts(ctypes.Structure):
    _fields_ = [("surf", IcpOpts), ("edge", IcpOpts), ("use_surf_points", ctypes.c_int32), ("use_edge_points", ctypes.c_int32),
                ("max_iteration", ctypes.c_int32), ("eps", ctypes.c_double)]


class PoolOpts(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_int32), ("prefetch", ctypes.c_int32), ("scans_per_job", ctypes.c_int32), ("chunk", ctypes.c_int32), ("matcher", ctypes.c_int32),
                ("max_points", ctypes.c_uint64), ("icp", IcpOpts)]


class Fitness(ctypes.Structure):
    _fields_ = [("score", ctypes.c_double), ("inliers", ctypes.c_int64), ("finite_points", ctypes.c_int64)]


class InitSearchOpts(ctypes.Structure):
    _fields_ = [("max_range", ctypes.c_double), ("min_inlier_ratio", ctypes.c_double)]


class SensorModelC(ctypes.Structure):
    """locgpu_sensor_model."""
    _fields_ = [("n_rings", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("range_scale", ctypes.c_float), ("min_range", ctypes.c_float),
                ("az_per_ring", ctypes.c_int32), ("reserved", ctypes.c_int32), ("cos_el", ctypes.c_void_p), ("sin_el", ctypes.c_void_p),
                ("cos_az", ctypes.c_void_p), ("sin_az", ctypes.c_void_p)]


class SweepMotionC(ctypes.Structure):
    """locgpu_sweep_motion."""
    _fields_ = [("n_knots", ctypes.c_int32), ("reserved", ctypes.c_int32), ("knot_times", ctypes.c_void_p), ("knot_poses", ctypes.c_void_p),
                ("ref_times", ctypes.c_void_p)]


TIME_NONE, TIME_F32, TIME_F64, TIME_U32 = 0, 1, 2, 3
RING_NONE, RING_U8, RING_U16 = 0, 1, 2
INTENSITY_NONE, INTENSITY_F32, INTENSITY_U8 = 0, 1, 2


class PointLayoutC(ctypes.Structure):
    """locgpu_point_layout: where the fields of a driver's point record are (PointCloud2::point_step and field offsets)."""
    _fields_ = [("stride_bytes", ctypes.c_uint32), ("xyz_offset", ctypes.c_uint32), ("time_offset", ctypes.c_uint32), ("time_kind", ctypes.c_uint32),
                ("ring_offset", ctypes.c_uint32), ("ring_kind", ctypes.c_uint32), ("intensity_offset", ctypes.c_uint32), ("intensity_kind", ctypes.c_uint32),
                ("min_range", ctypes.c_float), ("reserved", ctypes.c_uint32), ("time_scale", ctypes.c_double)]


def point_layout(layout, **kw):
    """A PointLayoutC from a layout given as plain data (a dict such as LAYOUT_VELODYNE, or a PointLayoutC), with fields overridden by
    keyword: stride_bytes, xyz_offset, time_offset, time_kind, ring_offset, ring_kind, intensity_offset, intensity_kind, min_range,
    time_scale. Missing fields: offsets 0, kinds NONE, min_range 4.0 (the reference's), time_scale 1."""
    if isinstance(layout, PointLayoutC):
        d = {name: getattr(layout, name) for name, _ in PointLayoutC._fields_}
    else:
        d = dict(min_range=4.0, time_scale=1.0)
        d.update(layout)
    d.update(kw)
    out = PointLayoutC()
    for k, v in d.items():
        if not hasattr(out, k):
            raise TypeError("unknown point layout field %r" % k)
        setattr(out, k, v)
    return out


# The reference's record types (LocUtils/include/LocUtils/common/point_types.h:99-169) as PCL lays them out, and a packed Velodyne record.
LAYOUT_VELODYNE = dict(stride_bytes=32, xyz_offset=0, intensity_offset=16, intensity_kind=INTENSITY_F32, time_offset=20, time_kind=TIME_F32, ring_offset=24,
                       ring_kind=RING_U16)
LAYOUT_RSLIDAR = dict(stride_bytes=32, xyz_offset=0, intensity_offset=16, intensity_kind=INTENSITY_F32, ring_offset=20, ring_kind=RING_U16, time_offset=24,
                      time_kind=TIME_F64)
LAYOUT_OUSTER = dict(stride_bytes=48, xyz_offset=0, intensity_offset=16, intensity_kind=INTENSITY_F32, time_offset=20, time_kind=TIME_U32, time_scale=1e-9,
                     ring_offset=26, ring_kind=RING_U8)
LAYOUT_VELODYNE_PACKED = dict(stride_bytes=22, xyz_offset=0, intensity_offset=12, intensity_kind=INTENSITY_F32, ring_offset=16, ring_kind=RING_U16, time_offset=18,
                              time_kind=TIME_F32)


def _records(layout, blob):
    """(uint8 array, number of records) of one blob: bytes, or any array whose bytes are the records."""
    a = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob).reshape(-1).view(np.uint8)
    if a.size % layout.stride_bytes:
        raise ValueError("a record blob holds whole records of %d bytes" % layout.stride_bytes)
    return a, a.size // layout.stride_bytes


class AlignStats(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("converged", ctypes.c_int32), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("last_effective_num", ctypes.c_int64), ("last_dx_norm", ctypes.c_double)]


def build(force=False):
    """Compile liblocgpu.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    """Load liblocgpu.so. Raises if it has not been built — the product path never falls back to the CPU."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LocGpuError(-2, "liblocgpu.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); no CPU fallback exists")
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, i32, dbl, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_float
        sig = {
            "locgpu_icp_opts_default": (None, [vp]), "locgpu_ndt_opts_default": (None, [vp]),
            "locgpu_create": (i32, [i32, vp]), "locgpu_destroy": (None, [vp]), "locgpu_last_error": (ctypes.c_char_p, [vp]),
            "locgpu_device_count": (i32, []),
            "locgpu_icp_set_target": (i32, [vp, vp, sz, sz]), "locgpu_icp_set_target_async": (i32, [vp, vp, sz, sz]), "locgpu_icp_target_info": (i32, [vp, vp]),
            "locgpu_knn": (i32, [vp, vp, sz, i32, i32, f32, i32, vp, vp]),
            "locgpu_icp_hb": (i32, [vp, vp, sz, sz, vp, vp, vp, vp, vp, vp]),
            "locgpu_icp_align": (i32, [vp, vp, sz, sz, vp, vp, vp, vp]),
            "locgpu_transform_cloud": (i32, [vp, vp, vp, sz, sz, vp, sz]),
            "locgpu_batch_create": (i32, [vp, vp, vp, sz, i32, vp]), "locgpu_batch_destroy": (None, [vp]),
            "locgpu_icp_align_batch": (i32, [vp, vp, vp, vp, vp, vp]), "locgpu_ndt_align_batch": (i32, [vp, vp, vp, vp, vp]),
            "locgpu_icp_align_batch_begin": (i32, [vp, vp, vp, vp]), "locgpu_ndt_align_batch_begin": (i32, [vp, vp, vp]),
            "locgpu_align_batch_end": (i32, [vp, vp, vp, vp]),
            "locgpu_icp_hb_batch": (i32, [vp, vp, vp, vp, vp]),
            "locgpu_gn_update": (i32, [vp, i32, i32, dbl, vp, vp, vp, vp]),
            "locgpu_ndt_set_target": (i32, [vp, vp, sz, sz, vp]), "locgpu_ndt_target_info": (i32, [vp, vp]),
            "locgpu_ndt_dump": (i32, [vp, vp, vp, vp, sz, vp]), "locgpu_debug_ndt_slots": (i32, [vp, vp, vp, sz, vp]), "locgpu_ndt_align": (i32, [vp, vp, sz, sz, vp, vp, vp]),
            "locgpu_profile_enable": (i32, [vp, i32]), "locgpu_profile_read": (i32, [vp, vp, i32]),
            "locgpu_visit_count_enable": (i32, [vp, i32]), "locgpu_visit_count_read": (i32, [vp, vp, i32]),
            "locgpu_search_stats_read": (i32, [vp, vp, i32]), "locgpu_debug_batch_nn": (i32, [vp, vp, i32, vp]), "locgpu_debug_batch_run_flags": (i32, [vp, vp, vp, vp]), "locgpu_debug_batch_slot": (i32, [vp]), "locgpu_graph_enable": (i32, [vp, i32]),
            "locgpu_debug_gn_solve": (i32, [vp, vp, i32, i32, i32, i32, dbl, i32, i32, i32, vp, i32, vp, vp, vp]),
            "locgpu_debug_loam_solve": (i32, [vp, vp, i32, vp, i32, i32, vp, dbl, i32, i32, vp, vp, vp]),
            "locgpu_cloud_create": (i32, [vp, vp]), "locgpu_cloud_destroy": (None, [vp]),
            "locgpu_cloud_upload": (i32, [vp, vp, sz, sz, sz, i32]), "locgpu_cloud_info": (i32, [vp, vp, vp]),
            "locgpu_cloud_download": (i32, [vp, vp, sz, sz, sz]), "locgpu_cloud_copy": (i32, [vp, vp]),
            "locgpu_cloud_remove_nan": (i32, [vp, vp]), "locgpu_cloud_voxel_filter": (i32, [vp, f32, vp, vp]),
            "locgpu_cloud_crop_box": (i32, [vp, vp, vp, vp]), "locgpu_cloud_transform": (i32, [vp, vp, vp]),
            "locgpu_cloud_append": (i32, [vp, vp]),
            "locgpu_icp_set_target_cloud": (i32, [vp, vp]), "locgpu_icp_set_target_cloud_async": (i32, [vp, vp]), "locgpu_ndt_set_target_cloud": (i32, [vp, vp, vp]),
            "locgpu_icp_align_cloud": (i32, [vp, vp, vp, vp, vp, vp]), "locgpu_ndt_align_cloud": (i32, [vp, vp, vp, vp, vp]),
            "locgpu_voxel_filter": (i32, [vp, vp, sz, sz, sz, i32, f32, vp, vp, vp]),
            "locgpu_crop_box": (i32, [vp, vp, sz, sz, sz, i32, vp, vp, vp, vp, vp]),
            "locgpu_remove_nan": (i32, [vp, vp, sz, sz, sz, i32, vp, vp, vp]),
            "locgpu_submap_create": (i32, [vp, i32, f32, vp]), "locgpu_submap_destroy": (None, [vp]),
            "locgpu_submap_add_keyframe": (i32, [vp, vp, vp]), "locgpu_submap_cloud": (i32, [vp, vp]),
            "locgpu_submap_last_keyframe": (i32, [vp, vp]), "locgpu_submap_info": (i32, [vp, vp, vp]),
            "locgpu_cloud_loam_extract": (i32, [vp, vp, i32, vp, vp]),
            "locgpu_loam_extract": (i32, [vp, vp, sz, sz, sz, i32, sz, i32, vp, vp, vp, vp, sz, sz]),
            "locgpu_batch_create_empty": (i32, [vp, i32, sz, vp]), "locgpu_batch_upload_async": (i32, [vp, vp, vp, sz]),
            "locgpu_batch_upload_wait": (i32, [vp]),
            "locgpu_comm_unique_id": (i32, [vp]), "locgpu_comm_init": (i32, [vp, i32, i32, vp]), "locgpu_comm_info": (i32, [vp, vp, vp]),
            "locgpu_batch_create_sharded": (i32, [vp, vp, vp, sz, i32, i32, i32, vp]),
            "locgpu_icp_set_target_bcast": (i32, [vp, vp, sz, sz, i32]),
            "locgpu_bfnn_set_target": (i32, [vp, vp, sz, sz]), "locgpu_bfnn_knn": (i32, [vp, vp, sz, i32, vp]),
            "locgpu_pool_opts_default": (None, [vp]), "locgpu_pool_create": (i32, [vp, vp, vp]), "locgpu_pool_destroy": (None, [vp]),
            "locgpu_pool_submit": (i32, [vp, vp, vp, sz, i32, i32, i32, vp, vp]), "locgpu_pool_wait": (i32, [vp, ctypes.c_int64, vp, vp]),
            "locgpu_pool_info": (i32, [vp, vp]), "locgpu_pool_profile_read": (i32, [vp, vp, i32]),
            "locgpu_pool_step": (i32, [vp, i32]), "locgpu_pool_done": (i32, [vp, ctypes.c_int64, vp]),
            "locgpu_icp_scan_match": (i32, [vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp, vp]),
            "locgpu_ndt_scan_match": (i32, [vp, vp, sz, sz, vp, vp, vp, vp, sz, vp, vp]),
            "locgpu_icp_fitness": (i32, [vp, vp, sz, sz, vp, i32, dbl, vp]), "locgpu_icp_fitness_batch": (i32, [vp, vp, vp, dbl, vp]),
            "locgpu_icp_fitness_resident": (i32, [vp, vp, dbl, vp]), "locgpu_batch_create_shared": (i32, [vp, vp, sz, sz, i32, vp]),
            "locgpu_init_search_opts_default": (None, [vp]),
            "locgpu_icp_init_search": (i32, [vp, vp, sz, sz, vp, i32, vp, vp, vp, vp, vp, vp]),
            "locgpu_pose_grid": (i32, [vp, dbl, dbl, dbl, dbl, vp, sz, vp]),
            "locgpu_ndt_fitness": (i32, [vp, vp, sz, sz, vp, i32, vp]), "locgpu_ndt_fitness_batch": (i32, [vp, vp, vp, vp]),
            "locgpu_ndt_fitness_resident": (i32, [vp, vp, vp]),
            "locgpu_ndt_hb": (i32, [vp, vp, sz, sz, vp, vp, vp, vp, vp]), "locgpu_ndt_hb_batch": (i32, [vp, vp, vp, vp]),
            "locgpu_ndt_init_search": (i32, [vp, vp, sz, sz, vp, i32, vp, vp, vp, vp, vp]),
            "locgpu_icp_build_map_planes": (i32, [vp]), "locgpu_icp_map_planes_info": (i32, [vp, vp]),
            "locgpu_icp_map_planes_dump": (i32, [vp, vp, vp, sz, vp]),
            "locgpu_loam_opts_default": (None, [vp]), "locgpu_loam_create": (i32, [i32, vp, vp]), "locgpu_loam_destroy": (None, [vp]),
            "locgpu_loam_last_error": (ctypes.c_char_p, [vp]), "locgpu_loam_set_target": (i32, [vp, vp, sz, vp, sz, sz]),
            "locgpu_loam_hb": (i32, [vp, vp, sz, vp, sz, sz, vp, vp, vp, vp, vp]),
            "locgpu_loam_scan_match": (i32, [vp, vp, sz, vp, sz, sz, vp, vp, vp, vp, sz]),
            "locgpu_loam_align_batch": (i32, [vp, i32, vp, vp, vp, vp, sz, vp, vp, vp]),
            "locgpu_loam_set_target_cloud": (i32, [vp, vp, vp]), "locgpu_loam_set_target_cloud_async": (i32, [vp, vp, vp]),
            "locgpu_loam_scan_match_cloud": (i32, [vp, vp, vp, vp, vp, vp, vp]), "locgpu_loam_fitness_resident": (i32, [vp, vp, dbl, vp]),
            "locgpu_loam_submap_create": (i32, [vp, i32, f32, vp]), "locgpu_loam_submap_destroy": (None, [vp]),
            "locgpu_loam_submap_add_keyframe": (i32, [vp, vp, vp, vp]), "locgpu_loam_submap_clouds": (i32, [vp, vp, vp]),
            "locgpu_loam_submap_info": (i32, [vp, vp, vp, vp]),
            "locgpu_loam_create_on": (i32, [vp, vp, vp, vp]),
            "locgpu_loam_fitness": (i32, [vp, vp, sz, vp, sz, sz, vp, i32, dbl, vp]),
            "locgpu_loam_fitness_cloud": (i32, [vp, vp, vp, vp, i32, dbl, vp]),
            "locgpu_loam_init_search": (i32, [vp, vp, sz, vp, sz, sz, vp, i32, vp, vp, vp, vp, vp]),
            "locgpu_loam_init_search_cloud": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
            "locgpu_batch_preprocess": (i32, [vp, f32, vp, vp, vp]), "locgpu_batch_upload_clouds": (i32, [vp, vp, i32]),
            "locgpu_batch_download_scan": (i32, [vp, i32, vp, sz, sz, vp]),
            "locgpu_batch_loam_extract": (i32, [vp, vp, i32, vp, vp, vp, vp, vp]), "locgpu_loam_align_batches": (i32, [vp, vp, vp, vp, vp, vp]),
            "locgpu_clouds_merge": (i32, [vp, vp, vp, i32, f32, vp, vp]), "locgpu_batch_merge": (i32, [vp, vp, vp, f32, vp, vp]),
            "locgpu_batch_export_cloud": (i32, [vp, i32, vp]),
            "locgpu_sensor_create": (i32, [vp, vp, vp]), "locgpu_sensor_destroy": (None, [vp]),
            "locgpu_batch_upload_ranges": (i32, [vp, vp, vp, vp]), "locgpu_batch_download_rings": (i32, [vp, i32, vp, sz, vp]),
            "locgpu_batch_loam_extract_resident": (i32, [vp, i32, vp, vp, vp, vp, vp]),
            "locgpu_cloud_upload_ranges": (i32, [vp, vp, vp, vp, vp]), "locgpu_range_ingest_times": (i32, [vp, vp]),
            "locgpu_sensor_set_col_times": (i32, [vp, vp]), "locgpu_batch_upload_ranges_deskew": (i32, [vp, vp, vp, vp, vp]),
            "locgpu_cloud_upload_ranges_deskew": (i32, [vp, vp, vp, vp, vp, vp]), "locgpu_range_deskew_matrices": (i32, [vp, i32, vp, sz, vp]),
            "locgpu_range_deskew_times": (i32, [vp, vp]),
            "locgpu_batch_upload_records": (i32, [vp, vp, vp, vp, vp]), "locgpu_batch_upload_records_deskew": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
            "locgpu_cloud_upload_records": (i32, [vp, vp, vp, ctypes.c_int64, vp, vp]),
            "locgpu_cloud_upload_records_deskew": (i32, [vp, vp, vp, ctypes.c_int64, dbl, vp, vp, vp]),
            "locgpu_records_deskew_debug": (i32, [vp, i32]), "locgpu_records_deskew_matrices": (i32, [vp, i32, vp, sz, vp]),
            "locgpu_records_ingest_times": (i32, [vp, vp]),
            "locgpu_batch_keep_times": (i32, [vp, i32]), "locgpu_batch_download_times": (i32, [vp, i32, vp, sz, vp]),
            "locgpu_batch_deskew": (i32, [vp, vp, vp, vp, vp]), "locgpu_batch_deskew_times": (i32, [vp, vp]),
            "locgpu_motion_from_poses": (i32, [vp, vp, i32, vp, vp]),
            "locgpu_icp_set_target_forest": (i32, [vp, vp, vp, i32, sz]), "locgpu_icp_set_target_forest_batch": (i32, [vp, vp]),
            "locgpu_icp_forest_info": (i32, [vp, vp, vp, vp]), "locgpu_icp_align_pairs": (i32, [vp, vp, vp, vp, vp, vp, vp]),
            "locgpu_icp_fitness_pairs": (i32, [vp, vp, vp, vp, dbl, vp]),
            "locgpu_ndt_set_target_set": (i32, [vp, vp, vp, i32, sz, vp]), "locgpu_ndt_set_target_set_batch": (i32, [vp, vp, vp]),
            "locgpu_ndt_set_info": (i32, [vp, vp, vp, vp]), "locgpu_ndt_set_dump": (i32, [vp, i32, vp, vp, vp, sz, vp]),
            "locgpu_ndt_align_pairs": (i32, [vp, vp, vp, vp, vp, vp]), "locgpu_ndt_fitness_pairs": (i32, [vp, vp, vp, vp, vp]),
            "locgpu_icp_set_target_forest_device": (i32, [vp, vp]), "locgpu_icp_set_target_cloud_device": (i32, [vp, vp]),
            "locgpu_icp_device_build_info": (i32, [vp, vp]), "locgpu_debug_tree_read": (i32, [vp, vp, sz, vp, sz]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def device_count():
    return int(lib().locgpu_device_count())


def comm_unique_id():
    """RCCL unique id (COMM_ID_BYTES bytes): make it on one rank, hand it to every rank's Context.comm_init."""
    buf = (ctypes.c_char * COMM_ID_BYTES)()
    rc = lib().locgpu_comm_unique_id(buf)
    if rc != 0:
        raise LocGpuError(rc, "locgpu_comm_unique_id failed")
    return bytes(buf)


def _cloud(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be [n, >=3] float32")
    return a


def _pose(p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.shape[-1] != 7:
        raise ValueError("pose must have 7 doubles (quaternion xyzw + translation)")
    return p


def icp_opts(method=P2P, **kw):
    o = IcpOpts()
    lib().locgpu_icp_opts_default(ctypes.byref(o))
    o.method = method
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown ICP option %r" % k)
        setattr(o, k, v)
    return o


def ndt_opts(**kw):
    o = NdtOpts()
    lib().locgpu_ndt_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown NDT option %r" % k)
        setattr(o, k, v)
    return o


def init_search_opts(**kw):
    o = InitSearchOpts()
    lib().locgpu_init_search_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown initial-pose search option %r" % k)
        setattr(o, k, v)
    return o


def loam_opts(**kw):
    """LoamOption's defaults (surface P2PLANE, edge P2LINE, 20 iterations, eps 1e-3, both classes on); `surf` / `edge` take IcpOpts."""
    o = LoamOpts()
    lib().locgpu_loam_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown LOAM option %r" % k)
        setattr(o, k, v)
    return o


def pose_grid(centre, xy_half, xy_step, yaw_half, yaw_step, cap=None):
    """Candidate poses around `centre` (locgpu_pose_grid; host only, needs no device): yaw-major, then x, then y.
    Returns (poses [min(count, cap), 7], count)."""
    c = _pose(centre)
    n = ctypes.c_size_t(0)
    rc = lib().locgpu_pose_grid(c.ctypes.data, xy_half, xy_step, yaw_half, yaw_step, None, 0, ctypes.byref(n))
    if rc != 0:
        raise LocGpuError(rc, "locgpu_pose_grid: bad arguments")
    k = n.value if cap is None else min(int(cap), n.value)
    out = np.zeros((k, 7))
    rc = lib().locgpu_pose_grid(c.ctypes.data, xy_half, xy_step, yaw_half, yaw_step, out.ctypes.data if k else None, k, ctypes.byref(n))
    if rc != 0:
        raise LocGpuError(rc, "locgpu_pose_grid: bad arguments")
    return out, int(n.value)


def _fitness_dict(f):
    return dict(score=f.score, inliers=int(f.inliers), finite_points=int(f.finite_points))


def _stats_dict(s):
    return dict(iterations=s.iterations, converged=bool(s.converged), status=s.status, last_effective_num=s.last_effective_num,
                last_dx_norm=s.last_dx_norm)


class Context:
    """One matcher instance on one GPU (what an IcpRegistration / NdtRegistration object owns)."""

    def __init__(self, device_id=0):
        self._h = ctypes.c_void_p()
        rc = lib().locgpu_create(device_id, ctypes.byref(self._h))
        if rc != 0:
            raise LocGpuError(rc, lib().locgpu_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().locgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise LocGpuError(rc, lib().locgpu_last_error(self._h).decode())

    # ---- IcpRegistration::SetInputTarget
    def icp_set_target(self, cloud, wait=True):
        """wait=False: returns once the points are copied; the host tree build runs on a worker thread and the next call that reads
        the ICP target completes the ingest."""
        c = _cloud(cloud)
        fn = lib().locgpu_icp_set_target if wait else lib().locgpu_icp_set_target_async
        self._check(fn(self._h, c.ctypes.data, c.shape[0], c.strides[0]))

    def icp_set_target_forest(self, clouds):
        """SetInputTarget of several clouds at once (locgpu_icp_set_target_forest): tree j is what icp_set_target(clouds[j]) builds;
        only icp_align_pairs / icp_fitness_pairs read such a target."""
        cs = [_cloud(c) for c in clouds]
        stride = next((c.strides[0] for c in cs if c.shape[0]), 16)
        if any(c.shape[0] and c.strides[0] != stride for c in cs):
            raise ValueError("all targets of a forest must share one point stride")
        ptrs = (ctypes.c_void_p * len(cs))(*[c.ctypes.data if c.shape[0] else None for c in cs])
        cnts = (ctypes.c_size_t * len(cs))(*[c.shape[0] for c in cs])
        self._check(lib().locgpu_icp_set_target_forest(self._h, ptrs, cnts, len(cs), stride))

    def icp_set_target_forest_batch(self, batch):
        """Target j = scan j of the resident plain batch (locgpu_icp_set_target_forest_batch)."""
        batch.upload_wait()
        self._check(lib().locgpu_icp_set_target_forest_batch(self._h, batch._h))

    def icp_set_target_forest_device(self, batch):
        """icp_set_target_forest_batch with the trees built on the device (locgpu_icp_set_target_forest_device)."""
        batch.upload_wait()
        self._check(lib().locgpu_icp_set_target_forest_device(self._h, batch._h))

    def icp_set_target_cloud_device(self, cloud):
        """icp_set_target_cloud with the tree built on the device (locgpu_icp_set_target_cloud_device)."""
        self._check(lib().locgpu_icp_set_target_cloud_device(self._h, cloud._h))

    def icp_device_build_info(self):
        """dict(path, first_degenerate, levels, tile, lane_len, threads, kind, bounded) — locgpu_icp_device_build_info."""
        out = np.zeros(8, dtype=np.int64)
        self._check(lib().locgpu_icp_device_build_info(self._h, out.ctypes.data))
        return dict(path=int(out[0]), first_degenerate=int(out[1]), levels=int(out[2]), tile=int(out[3]), lane_len=int(out[4]), threads=int(out[5]),
                    kind=int(out[6]), bounded=bool(out[7]))

    def debug_tree_read(self):
        """(slots uint64 [S + 2], leaf_slots uint32 [leaves] or None for a forest): the packed target as it stands in HBM, sentinel
        leaves and pads included (locgpu_debug_tree_read)."""
        info = np.zeros(4, dtype=np.int64)
        self._check(lib().locgpu_icp_target_info(self._h, info.ctypes.data))
        slots = np.zeros(int(info[3]) // 8 + 2, dtype=np.uint64)
        n = ctypes.c_int(0)
        forest = lib().locgpu_icp_forest_info(self._h, ctypes.byref(n), None, None) == 0
        leaves = None if forest else np.zeros(int(info[0]), dtype=np.uint32)
        self._check(lib().locgpu_debug_tree_read(self._h, slots.ctypes.data, slots.size, None if forest else leaves.ctypes.data, 0 if forest else leaves.size))
        return slots, leaves

    def icp_forest_info(self):
        """dict(n_targets, leaves [n], depth [n]) of the forest target (locgpu_icp_forest_info)."""
        n = ctypes.c_int(0)
        self._check(lib().locgpu_icp_forest_info(self._h, ctypes.byref(n), None, None))
        leaves = np.zeros(n.value, dtype=np.uint64)
        depth = np.zeros(n.value, dtype=np.int32)
        self._check(lib().locgpu_icp_forest_info(self._h, ctypes.byref(n), leaves.ctypes.data, depth.ctypes.data))
        return dict(n_targets=int(n.value), leaves=[int(v) for v in leaves], depth=[int(v) for v in depth])

    def icp_align_pairs(self, batch, target_of, init_poses, opts):
        """ScanMatch of scan i of the batch against target target_of[i] of the forest (-1: not aligned; locgpu_icp_align_pairs).
        init_poses None = the identity for every scan. Returns (poses [n, 7], stats)."""
        batch.upload_wait()
        t = np.ascontiguousarray(target_of, dtype=np.int32).reshape(batch.n_scans)
        ip = None if init_poses is None else _pose(init_poses).reshape(batch.n_scans, 7)
        out = np.zeros((batch.n_scans, 7))
        st = (AlignStats * batch.n_scans)()
        self._check(lib().locgpu_icp_align_pairs(self._h, batch._h, t.ctypes.data, None if ip is None else ip.ctypes.data, ctypes.byref(opts), out.ctypes.data, st))
        return out, [_stats_dict(s) for s in st]

    def icp_fitness_pairs(self, batch, target_of, poses, max_range=1.0, raw=False):
        """Score of scan i under poses[i] against target target_of[i] alone (locgpu_icp_fitness_pairs); -1: {+inf, 0, 0}."""
        batch.upload_wait()
        t = np.ascontiguousarray(target_of, dtype=np.int32).reshape(batch.n_scans)
        p = _pose(poses).reshape(batch.n_scans, 7)
        out = (Fitness * batch.n_scans)()
        self._check(lib().locgpu_icp_fitness_pairs(self._h, batch._h, t.ctypes.data, p.ctypes.data, max_range, out))
        return out if raw else [_fitness_dict(f) for f in out]

    def ndt_set_target_set(self, clouds, opts=None):
        """SetInputTarget of several clouds at once as a voxel set (locgpu_ndt_set_target_set): the grid of target j is what
        ndt_set_target(clouds[j], opts) builds; only ndt_align_pairs / ndt_fitness_pairs read such a target."""
        cs = [_cloud(c) for c in clouds]
        stride = next((c.strides[0] for c in cs if c.shape[0]), 16)
        if any(c.shape[0] and c.strides[0] != stride for c in cs):
            raise ValueError("all targets of a voxel set must share one point stride")
        ptrs = (ctypes.c_void_p * len(cs))(*[c.ctypes.data if c.shape[0] else None for c in cs])
        cnts = (ctypes.c_size_t * len(cs))(*[c.shape[0] for c in cs])
        self._check(lib().locgpu_ndt_set_target_set(self._h, ptrs, cnts, len(cs), stride, ctypes.byref(opts) if opts else None))

    def ndt_set_target_set_batch(self, batch, opts=None):
        """Target j = scan j of the resident plain batch, built on the device (locgpu_ndt_set_target_set_batch)."""
        batch.upload_wait()
        self._check(lib().locgpu_ndt_set_target_set_batch(self._h, batch._h, ctypes.byref(opts) if opts else None))

    def ndt_set_info(self):
        """dict(n_targets, points [n], voxels [n]) of the voxel-set target (locgpu_ndt_set_info)."""
        n = ctypes.c_int(0)
        self._check(lib().locgpu_ndt_set_info(self._h, ctypes.byref(n), None, None))
        points = np.zeros(n.value, dtype=np.uint64)
        voxels = np.zeros(n.value, dtype=np.uint64)
        self._check(lib().locgpu_ndt_set_info(self._h, ctypes.byref(n), points.ctypes.data, voxels.ctypes.data))
        return dict(n_targets=int(n.value), points=[int(v) for v in points], voxels=[int(v) for v in voxels])

    def ndt_set_dump(self, target):
        """(keys [n, 3], mu [n, 3], info [n, 3, 3]) of one target of the voxel set, in key order (locgpu_ndt_set_dump)."""
        n_out = ctypes.c_size_t(0)
        self._check(lib().locgpu_ndt_set_dump(self._h, target, None, None, None, 0, ctypes.byref(n_out)))
        n = int(n_out.value)
        keys = np.zeros((max(n, 1), 3), dtype=np.int32)
        mu = np.zeros((max(n, 1), 3))
        info = np.zeros((max(n, 1), 9))
        self._check(lib().locgpu_ndt_set_dump(self._h, target, keys.ctypes.data, mu.ctypes.data, info.ctypes.data, n, ctypes.byref(n_out)))
        return keys[:n], mu[:n], info[:n].reshape(n, 3, 3)

    def ndt_align_pairs(self, batch, target_of, init_poses=None):
        """ScanMatch of scan i of the batch against target target_of[i] of the voxel set (-1: not aligned; locgpu_ndt_align_pairs).
        init_poses None = the identity for every scan. Returns (poses [n, 7], stats)."""
        batch.upload_wait()
        t = np.ascontiguousarray(target_of, dtype=np.int32).reshape(batch.n_scans)
        ip = None if init_poses is None else _pose(init_poses).reshape(batch.n_scans, 7)
        out = np.zeros((batch.n_scans, 7))
        st = (AlignStats * batch.n_scans)()
        self._check(lib().locgpu_ndt_align_pairs(self._h, batch._h, t.ctypes.data, None if ip is None else ip.ctypes.data, out.ctypes.data, st))
        return out, [_stats_dict(s) for s in st]

    def ndt_fitness_pairs(self, batch, target_of, poses, raw=False):
        """Score of scan i under poses[i] against target target_of[i] alone (locgpu_ndt_fitness_pairs); -1: {+inf, 0, 0}."""
        batch.upload_wait()
        t = np.ascontiguousarray(target_of, dtype=np.int32).reshape(batch.n_scans)
        p = _pose(poses).reshape(batch.n_scans, 7)
        out = (Fitness * batch.n_scans)()
        self._check(lib().locgpu_ndt_fitness_pairs(self._h, batch._h, t.ctypes.data, p.ctypes.data, out))
        return out if raw else [_fitness_dict(f) for f in out]

    def icp_target_info(self):
        out = np.zeros(4, dtype=np.int64)
        self._check(lib().locgpu_icp_target_info(self._h, out.ctypes.data))
        return dict(num_leaves=int(out[0]), num_nodes=int(out[1]), depth=int(out[2]), bytes=int(out[3]))

    # ---- the plane table of P2PLANE_MAP (one math::FitPlane per map point at ingest)
    def icp_build_map_planes(self):
        self._check(lib().locgpu_icp_build_map_planes(self._h))

    def icp_map_planes_info(self):
        out = np.zeros(3, dtype=np.int64)
        self._check(lib().locgpu_icp_map_planes_info(self._h, out.ctypes.data))
        return dict(rows=int(out[0]), valid=int(out[1]), bytes=int(out[2]))

    def icp_map_planes_dump(self):
        """(n4 [n_points, 4] float64, valid [n_points] bool), rows by original point index of the target cloud."""
        n = ctypes.c_size_t(0)
        self._check(lib().locgpu_icp_map_planes_dump(self._h, None, None, 0, ctypes.byref(n)))  # size query
        n4 = np.zeros((max(n.value, 1), 4))
        valid = np.zeros(max(n.value, 1), dtype=np.uint8)
        self._check(lib().locgpu_icp_map_planes_dump(self._h, n4.ctypes.data, valid.ctypes.data, n4.shape[0], ctypes.byref(n)))
        return n4[:n.value], valid[:n.value].astype(bool)

    # ---- SearchPointInterface::FindNearstPoints, many queries
    def knn(self, queries, k=5, approximate=True, alpha=0.1, search_mode=SEARCH_TREE_FAITHFUL, with_visits=False):
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[:, :3])
        out = np.empty((q.shape[0], k), dtype=np.int32)
        vis = np.zeros((q.shape[0], 2), dtype=np.uint32) if with_visits else None
        self._check(lib().locgpu_knn(self._h, q.ctypes.data, q.shape[0], k, int(approximate), alpha, search_mode, out.ctypes.data,
                                     vis.ctypes.data if with_visits else None))
        return (out, vis) if with_visits else out

    # ---- BfnnRegistration (brute-force SearchPointInterface)
    def bfnn_set_target(self, cloud):
        c = _cloud(cloud)
        self._check(lib().locgpu_bfnn_set_target(self._h, c.ctypes.data, c.shape[0], c.strides[0]))

    def bfnn_knn(self, queries, k=5):
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[:, :3])
        out = np.empty((q.shape[0], k), dtype=np.int32)
        self._check(lib().locgpu_bfnn_knn(self._h, q.ctypes.data, q.shape[0], k, out.ctypes.data))
        return out

    # ---- MatchingInterface::CaculateMatrixHAndB
    def icp_hb(self, src, pose, opts):
        s = _cloud(src)
        H, B = np.zeros(36), np.zeros(6)
        eff, ok = ctypes.c_int64(0), ctypes.c_int(0)
        self._check(lib().locgpu_icp_hb(self._h, s.ctypes.data, s.shape[0], s.strides[0], _pose(pose).ctypes.data, ctypes.byref(opts),
                                        H.ctypes.data, B.ctypes.data, ctypes.byref(eff), ctypes.byref(ok)))
        return bool(ok.value), H.reshape(6, 6), B, int(eff.value)

    # ---- IcpRegistration::ScanMatch (pose part)
    def icp_align(self, src, init_pose, opts):
        s = _cloud(src)
        out = np.zeros(7)
        st = AlignStats()
        self._check(lib().locgpu_icp_align(self._h, s.ctypes.data, s.shape[0], s.strides[0], _pose(init_pose).ctypes.data, ctypes.byref(opts),
                                           out.ctypes.data, ctypes.byref(st)))
        return out, _stats_dict(st)

    # ---- IcpRegistration::ScanMatch whole: pose + output cloud (icp_registration.cpp:216-244)
    def icp_scan_match(self, src, init_pose, opts, in_place=False):
        """Returns (pose, stats, output cloud). The output cloud has the source's layout: every field of the source point, x, y, z
        replaced (pcl::transformPointCloud); in_place=True hands the source array itself as the output cloud."""
        s = _cloud(src)
        cloud = s if in_place else np.full_like(s, np.nan)
        out = np.zeros(7)
        st = AlignStats()
        self._check(lib().locgpu_icp_scan_match(self._h, s.ctypes.data, s.shape[0], s.strides[0], _pose(init_pose).ctypes.data, ctypes.byref(opts),
                                                out.ctypes.data, ctypes.byref(st), cloud.ctypes.data, cloud.strides[0], None, None))
        return out, _stats_dict(st), cloud

    # ---- NdtRegistration::ScanMatch whole (ndt_registration.cpp:238-261); result_pose in-out (status 1 leaves it as handed in)
    def ndt_scan_match(self, src, init_pose, result_pose=None):
        s = _cloud(src)
        cloud = np.full_like(s, np.nan)
        out = np.array(_pose(result_pose if result_pose is not None else init_pose), copy=True)
        st = AlignStats()
        self._check(lib().locgpu_ndt_scan_match(self._h, s.ctypes.data, s.shape[0], s.strides[0], _pose(init_pose).ctypes.data, out.ctypes.data,
                                                ctypes.byref(st), cloud.ctypes.data, cloud.strides[0], None, None))
        return out, _stats_dict(st), cloud

    # ---- pcl::transformPointCloud(src, out, pose.matrix().cast<float>())
    def transform_cloud(self, pose, src):
        s = _cloud(src)
        out = s.copy()
        self._check(lib().locgpu_transform_cloud(self._h, _pose(pose).ctypes.data, s.ctypes.data, s.shape[0], s.strides[0], out.ctypes.data,
                                                 out.strides[0]))
        return out

    # ---- filters either side of the matcher, host-pointer one-shots ([n, 4] float32 x, y, z, intensity)
    def _one_shot(self, fn, cloud, is_dense, *extra):
        a = _xyzi(cloud)
        out = np.zeros_like(a)
        n, d = ctypes.c_size_t(0), ctypes.c_int(0)
        self._check(fn(self._h, a.ctypes.data, a.shape[0], 16, 12, int(is_dense), *extra, out.ctypes.data, ctypes.byref(n), ctypes.byref(d)))
        return out[:n.value].copy(), bool(d.value)

    def voxel_filter(self, cloud, leaf, is_dense=True):
        return self._one_shot(lib().locgpu_voxel_filter, cloud, is_dense, float(leaf))

    def crop_box(self, cloud, mn, mx, is_dense=True):
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        return self._one_shot(lib().locgpu_crop_box, cloud, is_dense, mn.ctypes.data, mx.ctypes.data)

    def remove_nan(self, cloud, is_dense):
        return self._one_shot(lib().locgpu_remove_nan, cloud, is_dense)

    def loam_extract_full(self, full_points, num_scan=16):
        """One-shot on the reference's FullPointType records (64-byte structured array: x,y,z @0, uint8 intensity @24, ring @25)."""
        a = np.ascontiguousarray(full_points)
        if a.dtype.itemsize != 64:
            raise ValueError("FullPointType records are 64 bytes")
        n = len(a)
        edge, surf = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        ne, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(lib().locgpu_loam_extract(self._h, a.ctypes.data, n, 64, 24, 1, 25, int(num_scan), edge.ctypes.data, ctypes.byref(ne),
                                              surf.ctypes.data, ctypes.byref(ns), 16, 12))
        return edge[:ne.value].copy(), surf[:ns.value].copy()

    # ---- matcher entry points on resident clouds
    def icp_set_target_cloud(self, cloud, wait=True):
        """wait=False: the host tree build runs on a worker thread; the next call that reads the ICP target completes the ingest."""
        fn = lib().locgpu_icp_set_target_cloud if wait else lib().locgpu_icp_set_target_cloud_async
        self._check(fn(self._h, cloud._h))

    def ndt_set_target_cloud(self, cloud, opts=None):
        self._check(lib().locgpu_ndt_set_target_cloud(self._h, cloud._h, ctypes.byref(opts) if opts is not None else None))

    def icp_align_cloud(self, cloud, init_pose, opts):
        out = np.zeros(7)
        st = AlignStats()
        self._check(lib().locgpu_icp_align_cloud(self._h, cloud._h, _pose(init_pose).ctypes.data, ctypes.byref(opts), out.ctypes.data, ctypes.byref(st)))
        return out, _stats_dict(st)

    def ndt_align_cloud(self, cloud, init_pose):
        out = np.array(_pose(init_pose), copy=True)
        st = AlignStats()
        self._check(lib().locgpu_ndt_align_cloud(self._h, cloud._h, _pose(init_pose).ctypes.data, out.ctypes.data, ctypes.byref(st)))
        return out, _stats_dict(st)

    def clouds_merge(self, clouds, poses, leaf, out=None, with_passthrough=False):
        """Lio::GetGlobalMap on resident clouds (locgpu_clouds_merge): every cloud under its pose (``poses`` [n, 7], or None for clouds
        already in the world frame), joined in list order, one voxel filter (``leaf`` 0: join only). Clouds of other contexts on the
        GPU are accepted; ``out`` (a cloud of this context, none of the inputs; None = a new one) receives the map."""
        clouds = list(clouds)
        arr = (ctypes.c_void_p * max(len(clouds), 1))(*[c._h for c in clouds])
        p = None
        if poses is not None:
            p = _pose(poses).reshape(len(clouds), 7)
        out = out if out is not None else Cloud(self)
        pt = ctypes.c_int(0)
        self._check(lib().locgpu_clouds_merge(self._h, arr, p.ctypes.data if p is not None else None, len(clouds), float(leaf), out._h, ctypes.byref(pt)))
        return (out, bool(pt.value)) if with_passthrough else out

    # ---- several GPUs of one node: RCCL communicator + sharded batches
    def comm_init(self, rank, world, uid):
        """uid: COMM_ID_BYTES bytes from comm_unique_id() of one rank, handed to all (e.g. torch.distributed.broadcast)."""
        buf = (ctypes.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
        self._check(lib().locgpu_comm_init(self._h, int(rank), int(world), buf))

    def comm_info(self):
        r, w = ctypes.c_int(0), ctypes.c_int(1)
        self._check(lib().locgpu_comm_info(self._h, ctypes.byref(r), ctypes.byref(w)))
        return int(r.value), int(w.value)

    def icp_set_target_bcast(self, cloud, root=0):
        """Collective SetInputTarget: rank `root` builds the tree from its cloud and broadcasts it (other ranks may pass None)."""
        if cloud is None:
            self._check(lib().locgpu_icp_set_target_bcast(self._h, None, 0, 12, int(root)))
        else:
            c = _cloud(cloud)
            self._check(lib().locgpu_icp_set_target_bcast(self._h, c.ctypes.data, c.shape[0], c.strides[0], int(root)))

    # ---- batches
    def batch(self, scans, first=None, n_total=None):
        return Batch(self, scans, first=first, n_total=n_total)

    def batch_empty(self, n_scans, max_points):
        return Batch(self, None, n_scans=n_scans, max_points=max_points)

    def icp_align_batch(self, batch, init_poses, opts):
        batch.upload_wait()
        ip = _pose(init_poses).reshape(batch.n_scans, 7)
        out = np.zeros_like(ip)
        st = (AlignStats * batch.n_scans)()
        self._check(lib().locgpu_icp_align_batch(self._h, batch._h, ip.ctypes.data, ctypes.byref(opts), out.ctypes.data, st))
        return out, [_stats_dict(s) for s in st]

    def ndt_align_batch(self, batch, init_poses):
        batch.upload_wait()
        ip = _pose(init_poses).reshape(batch.n_scans, 7)
        out = np.zeros_like(ip)
        st = (AlignStats * batch.n_scans)()
        self._check(lib().locgpu_ndt_align_batch(self._h, batch._h, ip.ctypes.data, out.ctypes.data, st))
        return out, [_stats_dict(s) for s in st]

    # two batches in flight (locgpu.h: *_align_batch_begin / locgpu_align_batch_end)
    def icp_align_batch_begin(self, batch, init_poses, opts):
        batch.upload_wait()
        ip = _pose(init_poses).reshape(batch.n_scans, 7)
        self._check(lib().locgpu_icp_align_batch_begin(self._h, batch._h, ip.ctypes.data, ctypes.byref(opts)))

    def ndt_align_batch_begin(self, batch, init_poses):
        batch.upload_wait()
        ip = _pose(init_poses).reshape(batch.n_scans, 7)
        self._check(lib().locgpu_ndt_align_batch_begin(self._h, batch._h, ip.ctypes.data))

    def align_batch_end(self, batch):
        out = np.zeros((batch.n_scans, 7))
        st = (AlignStats * batch.n_scans)()
        self._check(lib().locgpu_align_batch_end(self._h, batch._h, out.ctypes.data, st))
        return out, [_stats_dict(s) for s in st]

    def icp_hb_batch(self, batch, poses, opts):
        batch.upload_wait()
        p = _pose(poses).reshape(batch.n_scans, 7)
        hb = np.zeros((batch.n_scans, 44))
        self._check(lib().locgpu_icp_hb_batch(self._h, batch._h, p.ctypes.data, ctypes.byref(opts), hb.ctypes.data))
        return hb

    # ---- MatchingInterface::GetFitnessScore, as pcl::Registration::getFitnessScore defines it (locgpu.h)
    def icp_fitness(self, src, poses, max_range=1.0, raw=False):
        """Score of one cloud under one pose ([7] → dict) or several ([n, 7] → list of dicts). raw=True: the ctypes array."""
        s = _cloud(src)
        p = _pose(poses)
        one = p.ndim == 1
        p = p.reshape(-1, 7)
        out = (Fitness * p.shape[0])()
        self._check(lib().locgpu_icp_fitness(self._h, s.ctypes.data, s.shape[0], s.strides[0], p.ctypes.data, p.shape[0], max_range, out))
        if raw:
            return out
        return _fitness_dict(out[0]) if one else [_fitness_dict(f) for f in out]

    def icp_fitness_batch(self, batch, poses, max_range=1.0, raw=False):
        batch.upload_wait()
        p = _pose(poses).reshape(batch.n_scans, 7)
        out = (Fitness * batch.n_scans)()
        self._check(lib().locgpu_icp_fitness_batch(self._h, batch._h, p.ctypes.data, max_range, out))
        return out if raw else [_fitness_dict(f) for f in out]

    def icp_fitness_resident(self, pose, max_range=1.0):
        """Score of the source cloud the last host-pointer single-scan call left in HBM (what the façade's GetFitnessScore uses)."""
        out = Fitness()
        self._check(lib().locgpu_icp_fitness_resident(self._h, _pose(pose).ctypes.data, max_range, ctypes.byref(out)))
        return _fitness_dict(out)

    def batch_shared(self, scan, n_entries):
        """A batch whose n_entries entries all read one resident copy of `scan` (locgpu_batch_create_shared)."""
        return Batch(self, None, n_scans=n_entries, shared=scan)

    # ---- initial-pose search: align from every candidate, score every result, pick the winner
    def icp_init_search(self, src, candidates, opts, sopts=None, raw=False):
        """Returns (poses [m, 7], fitness (list of dicts; raw=True: the ctypes array), stats, best index or -1)."""
        s = _cloud(src)
        c = _pose(candidates).reshape(-1, 7)
        m = c.shape[0]
        out = np.zeros((m, 7))
        fit = (Fitness * max(m, 1))()
        st = (AlignStats * max(m, 1))()
        best = ctypes.c_int(-2)
        self._check(lib().locgpu_icp_init_search(self._h, s.ctypes.data, s.shape[0], s.strides[0], c.ctypes.data, m, ctypes.byref(opts),
                                                 ctypes.byref(sopts) if sopts is not None else None, out.ctypes.data, fit, st, ctypes.byref(best)))
        return out, (fit if raw else [_fitness_dict(f) for f in fit]), [_stats_dict(x) for x in st], int(best.value)

    # ---- NdtRegistration
    def ndt_set_target(self, cloud, opts=None):
        c = _cloud(cloud)
        self._check(lib().locgpu_ndt_set_target(self._h, c.ctypes.data, c.shape[0], c.strides[0], ctypes.byref(opts) if opts else None))

    def ndt_target_info(self):
        out = np.zeros(3, dtype=np.int64)
        self._check(lib().locgpu_ndt_target_info(self._h, out.ctypes.data))
        return dict(num_voxels=int(out[0]), capacity=int(out[1]), bytes=int(out[2]))

    def ndt_dump(self):
        n = self.ndt_target_info()["num_voxels"]
        keys = np.zeros((max(n, 1), 3), dtype=np.int32)
        mu = np.zeros((max(n, 1), 3))
        info = np.zeros((max(n, 1), 9))
        n_out = ctypes.c_size_t(0)
        self._check(lib().locgpu_ndt_dump(self._h, keys.ctypes.data, mu.ctypes.data, info.ctypes.data, n, ctypes.byref(n_out)))
        return keys[:n], mu[:n], info[:n].reshape(n, 3, 3)

    def debug_ndt_slots(self):
        """(keys [cap] uint64, vid [cap] int32) of the slot array of the NDT target the context holds — direct, voxel set or incremental
        (locgpu_debug_ndt_slots): the raw key of every slot (all ones: free) and its record index (-1: free)."""
        n = ctypes.c_size_t(0)
        self._check(lib().locgpu_debug_ndt_slots(self._h, None, None, 0, ctypes.byref(n)))
        cap = int(n.value)
        keys = np.zeros(max(cap, 1), dtype=np.uint64)
        vid = np.zeros(max(cap, 1), dtype=np.int32)
        self._check(lib().locgpu_debug_ndt_slots(self._h, keys.ctypes.data, vid.ctypes.data, cap, ctypes.byref(n)))
        assert int(n.value) == cap
        return keys[:cap], vid[:cap]

    def ndt_align(self, src, init_pose):
        s = _cloud(src)
        out = np.zeros(7)
        st = AlignStats()
        self._check(lib().locgpu_ndt_align(self._h, s.ctypes.data, s.shape[0], s.strides[0], _pose(init_pose).ctypes.data, out.ctypes.data,
                                           ctypes.byref(st)))
        return out, _stats_dict(st)

    # ---- one iteration's H, B, effective_num, ok at a pose against the current NDT target, without the update
    def ndt_hb(self, src, pose):
        s = _cloud(src)
        H, B = np.zeros(36), np.zeros(6)
        eff, ok = ctypes.c_int64(0), ctypes.c_int(0)
        self._check(lib().locgpu_ndt_hb(self._h, s.ctypes.data, s.shape[0], s.strides[0], _pose(pose).ctypes.data, H.ctypes.data, B.ctypes.data,
                                        ctypes.byref(eff), ctypes.byref(ok)))
        return bool(ok.value), H.reshape(6, 6), B, int(eff.value)

    def ndt_hb_batch(self, batch, poses):
        batch.upload_wait()
        p = _pose(poses).reshape(batch.n_scans, 7)
        hb = np.zeros((batch.n_scans, 44))
        self._check(lib().locgpu_ndt_hb_batch(self._h, batch._h, p.ctypes.data, hb.ctypes.data))
        return hb

    # ---- the score and the candidate search against the direct NDT target (locgpu.h: score = mean χ² residual, dimensionless)
    def ndt_fitness(self, src, poses, raw=False):
        """Score of one cloud under one pose ([7] → dict) or several ([n, 7] → list of dicts). raw=True: the ctypes array."""
        s = _cloud(src)
        p = _pose(poses)
        one = p.ndim == 1
        p = p.reshape(-1, 7)
        out = (Fitness * max(p.shape[0], 1))()
        self._check(lib().locgpu_ndt_fitness(self._h, s.ctypes.data, s.shape[0], s.strides[0], p.ctypes.data, p.shape[0], out))
        if raw:
            return out
        return _fitness_dict(out[0]) if one else [_fitness_dict(f) for f in out]

    def ndt_fitness_batch(self, batch, poses, raw=False):
        batch.upload_wait()
        p = _pose(poses).reshape(batch.n_scans, 7)
        out = (Fitness * batch.n_scans)()
        self._check(lib().locgpu_ndt_fitness_batch(self._h, batch._h, p.ctypes.data, out))
        return out if raw else [_fitness_dict(f) for f in out]

    def ndt_fitness_resident(self, pose):
        """Score of the source cloud the last host-pointer single-scan call left in HBM (what the façade's GetFitnessScore uses)."""
        out = Fitness()
        self._check(lib().locgpu_ndt_fitness_resident(self._h, _pose(pose).ctypes.data, ctypes.byref(out)))
        return _fitness_dict(out)

    def ndt_init_search(self, src, candidates, sopts=None, raw=False):
        """Returns (poses [m, 7], fitness (list of dicts; raw=True: the ctypes array), stats, best index or -1)."""
        s = _cloud(src)
        c = _pose(candidates).reshape(-1, 7)
        m = c.shape[0]
        out = np.zeros((m, 7))
        fit = (Fitness * max(m, 1))()
        st = (AlignStats * max(m, 1))()
        best = ctypes.c_int(-2)
        self._check(lib().locgpu_ndt_init_search(self._h, s.ctypes.data, s.shape[0], s.strides[0], c.ctypes.data, m,
                                                 ctypes.byref(sopts) if sopts is not None else None, out.ctypes.data, fit, st, ctypes.byref(best)))
        return out, (fit if raw else [_fitness_dict(f) for f in fit]), [_stats_dict(x) for x in st], int(best.value)

    def graph_enable(self, on=True):
        """Replay a captured hipGraph of all Gauss–Newton iterations per align call (BASELINE config 5)."""
        self._check(lib().locgpu_graph_enable(self._h, int(on)))

    # ---- measurement hooks
    def profile_enable(self, on=True):
        self._check(lib().locgpu_profile_enable(self._h, int(on)))

    def profile_read(self, reset=True):
        out = np.zeros(6)
        self._check(lib().locgpu_profile_read(self._h, out.ctypes.data, int(reset)))
        return dict(search_ms=out[0], accum_ms=out[1], solve_ms=out[2], search_n=int(out[3]), accum_n=int(out[4]), solve_n=int(out[5]))

    def range_ingest_times(self):
        """(copy-stream ms, kernel ms) of the most recent upload_ranges while profile_enable is on (locgpu_range_ingest_times)."""
        out = np.zeros(2)
        self._check(lib().locgpu_range_ingest_times(self._h, out.ctypes.data))
        return float(out[0]), float(out[1])

    def range_deskew_times(self):
        """(copy-stream ms, matrix kernel ms, decode kernels ms) of the most recent upload_ranges_deskew while profile_enable is on
        (locgpu_range_deskew_times)."""
        out = np.zeros(3)
        self._check(lib().locgpu_range_deskew_times(self._h, out.ctypes.data))
        return float(out[0]), float(out[1]), float(out[2])

    def range_deskew_matrices(self, scan):
        """The [n_cols, 3, 4] float64 matrices of scan ``scan`` as the most recent deskewed ingest computed them (locgpu_range_deskew_matrices)."""
        n = ctypes.c_size_t(0)
        self._check(lib().locgpu_range_deskew_matrices(self._h, int(scan), None, 0, ctypes.byref(n)))
        out = np.zeros((int(n.value), 3, 4))
        self._check(lib().locgpu_range_deskew_matrices(self._h, int(scan), out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def records_deskew_debug(self, on=True):
        """Make the next upload_records_deskew calls keep each survivor's matrix for records_deskew_matrices (locgpu_records_deskew_debug)."""
        self._check(lib().locgpu_records_deskew_debug(self._h, int(on)))

    def records_deskew_matrices(self, scan):
        """The [n, 3, 4] float64 matrices of scan ``scan``'s survivors as the most recent deskewed record ingest with the debug switch on
        computed them (locgpu_records_deskew_matrices)."""
        n = ctypes.c_size_t(0)
        self._check(lib().locgpu_records_deskew_matrices(self._h, int(scan), None, 0, ctypes.byref(n)))
        out = np.zeros((int(n.value), 3, 4))
        self._check(lib().locgpu_records_deskew_matrices(self._h, int(scan), out.ctypes.data if out.size else None, out.size, ctypes.byref(n)))
        return out

    def records_ingest_times(self):
        """(copy-stream ms, kernel ms) of the most recent upload_records[_deskew] while profile_enable is on (locgpu_records_ingest_times)."""
        out = np.zeros(2)
        self._check(lib().locgpu_records_ingest_times(self._h, out.ctypes.data))
        return float(out[0]), float(out[1])

    def batch_deskew_times(self):
        """(check kernel ms, move kernel ms) of the most recent Batch.deskew while profile_enable is on (locgpu_batch_deskew_times)."""
        out = np.zeros(2)
        self._check(lib().locgpu_batch_deskew_times(self._h, out.ctypes.data))
        return float(out[0]), float(out[1])

    def visit_count_enable(self, on=True):
        self._check(lib().locgpu_visit_count_enable(self._h, int(on)))

    def visit_count_read(self, reset=True):
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().locgpu_visit_count_read(self._h, out.ctypes.data, int(reset)))
        return dict(nodes=int(out[0]), leaves=int(out[1]), queries=int(out[2]), distinct_slots=int(out[3]))


    def debug_batch_nn(self, batch, k=5):
        """Neighbour lists of the batch's most recent search stage as target point indices, [n_scans, max_points, k] (-1 = none)."""
        out = np.empty((batch.n_local, batch.max_points, k), dtype=np.int32)
        self._check(lib().locgpu_debug_batch_nn(self._h, batch._h, int(k), out.ctypes.data))
        return out  # rows beyond a scan's point count are -1: no search kernel writes them

    def debug_batch_run_flags(self, batch):
        """Run flags of the batch's most recent search stage: (words [n_scans, ceil(max_points / 64)] uint64 — bit j of word w set:
        point 64 w + j leads a run of equal neighbour sets, clear: it follows the point before it — and whether that stage wrote
        any; words of 64-point groups wholly past a scan's count are never written)."""
        out = np.zeros((batch.n_local, (batch.max_points + 63) // 64), dtype=np.uint64)
        written = ctypes.c_int(0)
        self._check(lib().locgpu_debug_batch_run_flags(self._h, batch._h, out.ctypes.data, ctypes.byref(written)))
        return out, bool(written.value)

    def debug_gn_solve(self, partials, state, method, min_effective_pts=10, eps=1e-2, max_iteration=20, do_update=True, two_stage=False,
                       scans=None, hb=None):
        """The production solve stage on chosen block partials (locgpu_debug_gn_solve). partials [n_scans, blocks_per_scan, ACC_W] float64,
        state [n_scans] SOLVE_STATE, scans: optional list — block i solves scan scans[i]; hb: optional [n_scans, HB_W] start contents (rows
        no block writes come back unchanged; default NaN). Returns (state_out [n_scans] SOLVE_STATE, hb [n_scans, HB_W])."""
        p = np.ascontiguousarray(partials, dtype=np.float64)
        if p.ndim != 3 or p.shape[2] != ACC_W:
            raise ValueError("partials must be [n_scans, blocks_per_scan, %d]" % ACC_W)
        n, blocks = p.shape[0], p.shape[1]
        st_in = np.ascontiguousarray(state, dtype=SOLVE_STATE).reshape(n)
        st_out = np.zeros(n, dtype=SOLVE_STATE)
        hb_out = np.full((n, HB_W), np.nan) if hb is None else np.array(hb, dtype=np.float64, copy=True).reshape(n, HB_W)
        sc = None if scans is None else np.ascontiguousarray(scans, dtype=np.int32)
        self._check(lib().locgpu_debug_gn_solve(self._h, p.ctypes.data, n, blocks, int(method), int(min_effective_pts), float(eps), int(max_iteration),
                                                int(bool(do_update)), int(bool(two_stage)), None if sc is None else sc.ctypes.data,
                                                0 if sc is None else len(sc), st_in.ctypes.data, st_out.ctypes.data, hb_out.ctypes.data))
        return st_out, hb_out

    def debug_loam_solve(self, partials_surf, partials_edge, state, min_effective_pts=(10, 10), eps=1e-3, max_iteration=20, do_update=True, hb=None):
        """The production LOAM solve on chosen block partials of the two classes (locgpu_debug_loam_solve); None switches a class off.
        Returns (state_out [n_scans] SOLVE_STATE, hb [n_scans, LOAM_HB_W])."""
        parts = [None if p is None else np.ascontiguousarray(p, dtype=np.float64) for p in (partials_surf, partials_edge)]
        for p in parts:
            if p is not None and (p.ndim != 3 or p.shape[2] != ACC_W):
                raise ValueError("partials must be [n_scans, blocks_per_scan, %d]" % ACC_W)
        n = len(state)
        if any(p is not None and p.shape[0] != n for p in parts):
            raise ValueError("every class needs a row set per scan")
        st_in = np.ascontiguousarray(state, dtype=SOLVE_STATE).reshape(n)
        st_out = np.zeros(n, dtype=SOLVE_STATE)
        hb_out = np.full((n, LOAM_HB_W), np.nan) if hb is None else np.array(hb, dtype=np.float64, copy=True).reshape(n, LOAM_HB_W)
        mins = np.ascontiguousarray(min_effective_pts, dtype=np.int32).reshape(2)
        self._check(lib().locgpu_debug_loam_solve(self._h, None if parts[0] is None else parts[0].ctypes.data, 0 if parts[0] is None else parts[0].shape[1],
                                                  None if parts[1] is None else parts[1].ctypes.data, 0 if parts[1] is None else parts[1].shape[1], n,
                                                  mins.ctypes.data, float(eps), int(max_iteration), int(bool(do_update)), st_in.ctypes.data,
                                                  st_out.ctypes.data, hb_out.ctypes.data))
        return st_out, hb_out

    def search_stats_read(self, reset=True):
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().locgpu_search_stats_read(self._h, out.ctypes.data, int(reset)))
        return dict(searched=int(out[0]), redone=int(out[1]), walked=int(out[2]), replayed=int(out[3]))


def _xyzi(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("cloud must be [n, 4] float32 (x, y, z, intensity)")
    return a


class Cloud:
    """A cloud resident in HBM (locgpu_cloud): float32 x, y, z, intensity per point + PCL's is_dense flag."""

    def __init__(self, ctx, points=None, is_dense=True, _borrowed=None):
        self.ctx = ctx
        self._owned = _borrowed is None
        if _borrowed is not None:
            self._h = _borrowed
        else:
            self._h = ctypes.c_void_p()
            ctx._check(lib().locgpu_cloud_create(ctx._h, ctypes.byref(self._h)))
            if points is not None:
                self.upload(points, is_dense)

    def upload(self, points, is_dense=True):
        a = _xyzi(points)
        self.ctx._check(lib().locgpu_cloud_upload(self._h, a.ctypes.data, a.shape[0], 16, 12, int(is_dense)))
        return self

    @property
    def info(self):
        n, d = ctypes.c_size_t(0), ctypes.c_int(0)
        self.ctx._check(lib().locgpu_cloud_info(self._h, ctypes.byref(n), ctypes.byref(d)))
        return int(n.value), bool(d.value)

    def __len__(self):
        return self.info[0]

    @property
    def is_dense(self):
        return self.info[1]

    def download(self):
        n = len(self)
        out = np.zeros((n, 4), np.float32)
        self.ctx._check(lib().locgpu_cloud_download(self._h, out.ctypes.data, n, 16, 12))
        return out

    def _out(self, out):
        return out if out is not None else Cloud(self.ctx)

    def copy(self, out=None):
        out = self._out(out)
        self.ctx._check(lib().locgpu_cloud_copy(self._h, out._h))
        return out

    def remove_nan(self, out=None):
        out = self._out(out)
        self.ctx._check(lib().locgpu_cloud_remove_nan(self._h, out._h))
        return out

    def voxel_filter(self, leaf, out=None, with_passthrough=False):
        out = self._out(out)
        pt = ctypes.c_int(0)
        self.ctx._check(lib().locgpu_cloud_voxel_filter(self._h, float(leaf), out._h, ctypes.byref(pt)))
        return (out, bool(pt.value)) if with_passthrough else out

    def crop_box(self, mn, mx, out=None):
        out = self._out(out)
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        self.ctx._check(lib().locgpu_cloud_crop_box(self._h, mn.ctypes.data, mx.ctypes.data, out._h))
        return out

    def transform(self, pose, out=None):
        out = self._out(out)
        self.ctx._check(lib().locgpu_cloud_transform(self._h, _pose(pose).ctypes.data, out._h))
        return out

    def append(self, other):
        self.ctx._check(lib().locgpu_cloud_append(self._h, other._h))
        return self

    def upload_ranges(self, sensor, image, with_rings=True):
        """Decode one range image into the cloud (locgpu_cloud_upload_ranges: CloudConver::Conver's rules on the device, intensity 0,
        is_dense). Returns the survivors' ring bytes (uint8, one per point) — what loam_extract takes — or None."""
        img = sensor.model.image(image)
        rings = np.zeros(sensor.model.cells, np.uint8) if with_rings else None
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_cloud_upload_ranges(self._h, sensor._h, img.ctypes.data, rings.ctypes.data if with_rings else None, ctypes.byref(n)))
        return np.ascontiguousarray(rings[:int(n.value)]) if with_rings else None

    def upload_ranges_deskew(self, sensor, image, knot_times, knot_poses, ref_time, with_rings=True):
        """upload_ranges with the scan motion-compensated per column (locgpu_cloud_upload_ranges_deskew): knot_times [K], knot_poses
        [K, 7] (the sensor's pose, quaternion xyzw + translation), ref_time the instant whose sensor frame the cloud is expressed in."""
        img = sensor.model.image(image)
        motion, keep = sweep_motion(1, knot_times, knot_poses, [ref_time])
        rings = np.zeros(sensor.model.cells, np.uint8) if with_rings else None
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_cloud_upload_ranges_deskew(self._h, sensor._h, img.ctypes.data, ctypes.byref(motion), rings.ctypes.data if with_rings else None,
                                                                ctypes.byref(n)))
        return np.ascontiguousarray(rings[:int(n.value)]) if with_rings else None

    def upload_records(self, layout, blob, with_rings=True):
        """Conver on the device for one blob of point records into the cloud (locgpu_cloud_upload_records: intensity kept, is_dense).
        Returns the survivors' ring bytes (uint8, one per point), or None without them or for a layout without a ring field."""
        L = point_layout(layout)
        a, n_rec = _records(L, blob)
        with_rings = with_rings and L.ring_kind != RING_NONE
        rings = np.zeros(max(n_rec, 1), np.uint8) if with_rings else None
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_cloud_upload_records(self._h, ctypes.byref(L), a.ctypes.data if n_rec else None, n_rec, rings.ctypes.data if with_rings else None,
                                                          ctypes.byref(n)))
        return np.ascontiguousarray(rings[:int(n.value)]) if with_rings else None

    def upload_records_deskew(self, layout, blob, time_offset, knot_times, knot_poses, ref_time, with_rings=True):
        """upload_records with every survivor motion-compensated at its own time (locgpu_cloud_upload_records_deskew): the point's time is
        field * layout.time_scale + time_offset on the clock of knot_times [K]; knot_poses [K, 7]; ref_time as in upload_ranges_deskew."""
        L = point_layout(layout)
        a, n_rec = _records(L, blob)
        motion, keep = sweep_motion(1, knot_times, knot_poses, [ref_time])
        with_rings = with_rings and L.ring_kind != RING_NONE
        rings = np.zeros(max(n_rec, 1), np.uint8) if with_rings else None
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_cloud_upload_records_deskew(self._h, ctypes.byref(L), a.ctypes.data if n_rec else None, n_rec, float(time_offset), ctypes.byref(motion),
                                                                 rings.ctypes.data if with_rings else None, ctypes.byref(n)))
        return np.ascontiguousarray(rings[:int(n.value)]) if with_rings else None

    def loam_extract(self, ring, num_scan=16):
        """LoamFeatureExtract::Extract on a resident cloud: returns (edge, surf) resident clouds."""
        ring = np.ascontiguousarray(ring, dtype=np.uint8)
        if len(ring) != len(self):
            raise ValueError("one ring byte per point")
        edge, surf = Cloud(self.ctx), Cloud(self.ctx)
        self.ctx._check(lib().locgpu_cloud_loam_extract(self._h, ring.ctypes.data, int(num_scan), edge._h, surf._h))
        return edge, surf

    def close(self):
        if self._owned and getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().locgpu_cloud_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


class SensorModel:
    """A range-image sensor on the host (locgpu_sensor_model): sizes, range_scale, min_range and the caller's float32 tables —
    cos_el / sin_el [n_rings]; cos_az / sin_az [n_cols], or [n_rings, n_cols] for per-laser azimuth offsets (az_per_ring)."""

    def __init__(self, n_rings, n_cols, range_scale, min_range, cos_el, sin_el, cos_az, sin_az):
        self.n_rings, self.n_cols = int(n_rings), int(n_cols)
        self.range_scale, self.min_range = np.float32(range_scale), np.float32(min_range)
        self.cos_el, self.sin_el, self.cos_az, self.sin_az = (np.ascontiguousarray(t, dtype=np.float32) for t in (cos_el, sin_el, cos_az, sin_az))
        self.az_per_ring = int(self.cos_az.ndim == 2)
        want_az = (self.n_rings, self.n_cols) if self.az_per_ring else (self.n_cols,)
        if self.cos_el.shape != (self.n_rings,) or self.sin_el.shape != (self.n_rings,) or self.cos_az.shape != want_az or self.sin_az.shape != want_az:
            raise ValueError("sensor tables do not match n_rings / n_cols")

    @property
    def cells(self):
        return self.n_rings * self.n_cols

    def c_struct(self):
        return SensorModelC(self.n_rings, self.n_cols, float(self.range_scale), float(self.min_range), self.az_per_ring, 0, self.cos_el.ctypes.data,
                            self.sin_el.ctypes.data, self.cos_az.ctypes.data, self.sin_az.ctypes.data)

    def image(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint16)
        if a.size != self.cells:
            raise ValueError("a range image of this sensor has %d x %d cells" % (self.n_rings, self.n_cols))
        return a


def sweep_motion(n_scans, knot_times, knot_poses, ref_times):
    """(locgpu_sweep_motion, the arrays it points into) for n_scans scans: knot_times [n_scans, K], knot_poses [n_scans, K, 7], ref_times
    [n_scans], all float64. Keep the second value alive while the struct is in use."""
    t = np.ascontiguousarray(knot_times, dtype=np.float64).reshape(n_scans, -1)
    p = np.ascontiguousarray(knot_poses, dtype=np.float64).reshape(n_scans, -1)
    r = np.ascontiguousarray(ref_times, dtype=np.float64).reshape(-1)
    if p.shape[1] != 7 * t.shape[1] or len(r) != n_scans:
        raise ValueError("a sweep motion holds K times and K poses of 7 per scan, and one reference time per scan")
    return SweepMotionC(t.shape[1], 0, t.ctypes.data, p.ctypes.data, r.ctypes.data), (t, p, r)


def motion_from_poses(poses, stamps):
    """(knot_times [n, 3], knot_poses [n, 3, 7]) of n consecutive scans from their poses [n, 7] (quaternion xyzw + translation) and
    strictly increasing stamps [n] (locgpu_motion_from_poses, host only): scan i gets the poses of scans i-1, i, i+1, a missing
    neighbour extrapolated at constant velocity as the reference's predict_pos. With ref_times they are what Batch.deskew takes."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    t = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1)
    if len(t) != len(p):
        raise ValueError("one stamp per pose")
    n = len(p)
    kt, kp = np.zeros((n, 3), np.float64), np.zeros((n, 3, 7), np.float64)
    rc = lib().locgpu_motion_from_poses(p.ctypes.data if n else None, t.ctypes.data if n else None, n, kt.ctypes.data if n else None, kp.ctypes.data if n else None)
    if rc != 0:
        raise LocGpuError(rc, lib().locgpu_last_error(None).decode())
    return kt, kp


class Sensor:
    """A sensor model resident in HBM (locgpu_sensor): what Batch.upload_ranges and Cloud.upload_ranges decode with."""

    def __init__(self, ctx, model):
        self.ctx, self.model = ctx, model
        self._h = ctypes.c_void_p()
        m = model.c_struct()
        ctx._check(lib().locgpu_sensor_create(ctx._h, ctypes.byref(m), ctypes.byref(self._h)))

    def set_col_times(self, col_time):
        """The firing time of every column, seconds from the scan's time origin (locgpu_sensor_set_col_times); what the deskewed
        ingests look the sensor's pose up with."""
        t = np.ascontiguousarray(col_time, dtype=np.float64)
        if t.shape != (self.model.n_cols,):
            raise ValueError("one time per column: %d" % self.model.n_cols)
        self.ctx._check(lib().locgpu_sensor_set_col_times(self._h, t.ctypes.data))

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().locgpu_sensor_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


class Submap:
    """Lio::AddCloud's keyframe local map in HBM (locgpu_submap)."""

    def __init__(self, ctx, num_kfs, leaf):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        ctx._check(lib().locgpu_submap_create(ctx._h, int(num_kfs), float(leaf), ctypes.byref(self._h)))

    def add_keyframe(self, scan, pose=None):
        self.ctx._check(lib().locgpu_submap_add_keyframe(self._h, scan._h, _pose(pose).ctypes.data if pose is not None else None))

    def cloud(self):
        h = ctypes.c_void_p()
        self.ctx._check(lib().locgpu_submap_cloud(self._h, ctypes.byref(h)))
        return Cloud(self.ctx, _borrowed=h)

    def last_keyframe(self):
        h = ctypes.c_void_p()
        self.ctx._check(lib().locgpu_submap_last_keyframe(self._h, ctypes.byref(h)))
        return Cloud(self.ctx, _borrowed=h)

    @property
    def info(self):
        k, n = ctypes.c_int(0), ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_submap_info(self._h, ctypes.byref(k), ctypes.byref(n)))
        return int(k.value), int(n.value)

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().locgpu_submap_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


class LoamSubmap:
    """The pair of keyframe local maps of Lio::AddCloud(FullCloudPtr) in HBM (locgpu_loam_submap, lio.cpp:331-409): one queue length for
    both classes; the first keyframe seeds both maps unfiltered, every later one is appended (or the maps rebuilt) and filtered."""

    def __init__(self, ctx, num_kfs, leaf):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        ctx._check(lib().locgpu_loam_submap_create(ctx._h, int(num_kfs), float(leaf), ctypes.byref(self._h)))

    def add_keyframe(self, edge, surf, pose=None):
        self.ctx._check(lib().locgpu_loam_submap_add_keyframe(self._h, edge._h, surf._h, _pose(pose).ctypes.data if pose is not None else None))

    def clouds(self):
        """(edge map, surface map), borrowed: what Loam.set_target_cloud takes."""
        e, s = ctypes.c_void_p(), ctypes.c_void_p()
        self.ctx._check(lib().locgpu_loam_submap_clouds(self._h, ctypes.byref(e), ctypes.byref(s)))
        return Cloud(self.ctx, _borrowed=e), Cloud(self.ctx, _borrowed=s)

    @property
    def info(self):
        """(keyframes, edge map points, surface map points)"""
        k, ne, ns = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_loam_submap_info(self._h, ctypes.byref(k), ctypes.byref(ne), ctypes.byref(ns)))
        return int(k.value), int(ne.value), int(ns.value)

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().locgpu_loam_submap_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


class MarshalledScans:
    """The (pointer, count) arrays of a list of host scans, built once: what a C/C++ caller of locgpu_batch_upload_async holds
    anyway. Pass it wherever a list of scans is accepted to skip the per-call Python marshalling (≈0.4 ms for 256 scans)."""

    def __init__(self, scans):
        self.scans, self.ptrs, self.cnts, self.stride = Batch._marshal(list(scans))

    def __len__(self):
        return len(self.scans)


class Batch:
    """A batch of scans resident in HBM (locgpu_batch). ``n_scans`` = the scans poses are kept for (all n_total of a sharded batch)."""

    def __init__(self, ctx, scans, first=None, n_total=None, n_scans=None, max_points=None, shared=None):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        self._keep = None
        if shared is not None:  # n_scans entries that all read one resident copy of `shared`
            c = _cloud(shared)
            self.n_local = self.n_scans = int(n_scans)
            self.max_points = c.shape[0]
            ctx._check(lib().locgpu_batch_create_shared(ctx._h, c.ctypes.data, c.shape[0], c.strides[0], self.n_scans, ctypes.byref(self._h)))
            return
        if scans is None:  # capacity only; fill with upload_async
            self.n_local = self.n_scans = int(n_scans)
            self.max_points = int(max_points)
            ctx._check(lib().locgpu_batch_create_empty(ctx._h, self.n_scans, int(max_points), ctypes.byref(self._h)))
            return
        if n_total is not None and len(scans) == 0:  # a rank that holds none of the batch's scans still takes part in its collectives
            self.n_local, self.max_points, self.n_scans = 0, 0, int(n_total)
            ctx._check(lib().locgpu_batch_create_sharded(ctx._h, None, None, 16, 0, int(first or 0), self.n_scans, ctypes.byref(self._h)))
            return
        scans, ptrs, cnts, stride = self._marshal(scans)
        self.n_local = len(scans)
        self.max_points = max(s.shape[0] for s in scans)
        if n_total is None:
            self.n_scans = self.n_local
            ctx._check(lib().locgpu_batch_create(ctx._h, ptrs, cnts, stride, self.n_local, ctypes.byref(self._h)))
        else:  # sharded: this rank holds scans [first, first + len(scans)) of n_total
            self.n_scans = int(n_total)
            ctx._check(lib().locgpu_batch_create_sharded(ctx._h, ptrs, cnts, stride, self.n_local, int(first or 0), self.n_scans, ctypes.byref(self._h)))

    @staticmethod
    def _marshal(scans):
        if isinstance(scans, MarshalledScans):
            return scans.scans, scans.ptrs, scans.cnts, scans.stride
        scans = [_cloud(s) for s in scans]
        if not scans:
            raise ValueError("empty batch")
        stride = next((s.strides[0] for s in scans if s.shape[0]), 16)  # an empty scan has no stride of its own
        if any(s.shape[0] and s.strides[0] != stride for s in scans):
            raise ValueError("all scans of a batch must share one point stride")
        ptrs = (ctypes.c_void_p * len(scans))(*[s.ctypes.data for s in scans])
        cnts = (ctypes.c_size_t * len(scans))(*[s.shape[0] for s in scans])
        return scans, ptrs, cnts, stride

    def upload_async(self, scans):
        """Replace the batch's scans; returns at once (the copy runs beside the GPU's current work). The arrays are kept
        alive here until upload_wait() / the next align call on this batch."""
        self.upload_wait()
        scans, ptrs, cnts, stride = self._marshal(scans)
        if len(scans) != self.n_local:
            raise ValueError("upload_async needs %d scans" % self.n_local)
        self._keep = (scans, ptrs, cnts)
        self.ctx._check(lib().locgpu_batch_upload_async(self._h, ptrs, cnts, stride))

    def debug_slot(self):
        """Index of the compute stream the batch's current or last alignment uses (locgpu_debug_batch_slot)."""
        return int(lib().locgpu_debug_batch_slot(self._h))

    def upload_wait(self):
        if self._keep is not None:
            rc = lib().locgpu_batch_upload_wait(self._h)
            self._keep = None
            self.ctx._check(rc)

    def preprocess(self, leaf, out=None):
        """RemoveNanPoint → VoxelFilter::Filter on every scan of the batch in one pass (locgpu_batch_preprocess), into ``out`` (a batch
        of the same context and n_scans; None = in place). Returns (counts, status) as int32 arrays; when a filtered scan does not fit
        ``out`` the LocGpuError carries the needed counts as ``.counts``."""
        self.upload_wait()
        dst = self if out is None else out
        dst.upload_wait()
        counts, status = np.zeros(self.n_local, np.int32), np.zeros(self.n_local, np.int32)
        rc = lib().locgpu_batch_preprocess(self._h, float(leaf), dst._h, counts.ctypes.data, status.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.counts = counts
            raise err
        return counts, status

    def loam_extract(self, rings, num_scan, edge, surf):
        """The LOAM feature picker on every scan of the batch in one pass (locgpu_batch_loam_extract): scan s of ``edge`` / ``surf``
        (two other batches of the same context and n_scans) becomes Cloud.loam_extract of scan s with ``rings[s]`` (uint8, one per
        point). Returns (edge counts, surface counts, status) as int32 arrays; a refused call raises a LocGpuError that carries the
        needed counts and the per-scan status as ``.edge_counts``, ``.surf_counts`` and ``.status``."""
        self.upload_wait()
        edge.upload_wait()
        surf.upload_wait()
        rings = [np.ascontiguousarray(r, dtype=np.uint8) if r is not None else None for r in rings]
        if len(rings) != self.n_local:
            raise ValueError("loam_extract needs %d ring arrays" % self.n_local)
        ptrs = (ctypes.c_void_p * max(len(rings), 1))(*[(r.ctypes.data if r is not None and r.size else None) for r in rings])
        ne, ns, status = (np.zeros(self.n_local, np.int32) for _ in range(3))
        rc = lib().locgpu_batch_loam_extract(self._h, ptrs, int(num_scan), edge._h, surf._h, ne.ctypes.data, ns.ctypes.data, status.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.edge_counts, err.surf_counts, err.status = ne, ns, status
            raise err
        return ne, ns, status

    def upload_ranges(self, sensor, images):
        """Replace the batch's scans by the decoded range images (locgpu_batch_upload_ranges: one uint16 image of the sensor's
        n_rings x n_cols cells per scan; CloudConver::Conver's rules on the device) and leave their ring bytes resident. Blocking.
        Returns the counts; when a scan does not fit the batch the LocGpuError carries the needed counts as ``.counts``."""
        self.upload_wait()
        images = [sensor.model.image(a) for a in images]
        if len(images) != self.n_local:
            raise ValueError("upload_ranges needs %d images" % self.n_local)
        ptrs = (ctypes.c_void_p * max(len(images), 1))(*[a.ctypes.data for a in images])
        counts = np.zeros(self.n_local, np.int32)
        rc = lib().locgpu_batch_upload_ranges(self._h, sensor._h, ptrs, counts.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.counts = counts
            raise err
        return counts

    def upload_ranges_deskew(self, sensor, images, knot_times, knot_poses, ref_times):
        """upload_ranges with every scan motion-compensated per column (locgpu_batch_upload_ranges_deskew): knot_times [n, K],
        knot_poses [n, K, 7] (the sensor's pose at each knot, quaternion xyzw + translation), ref_times [n]. Same returns and errors."""
        self.upload_wait()
        images = [sensor.model.image(a) for a in images]
        if len(images) != self.n_local:
            raise ValueError("upload_ranges_deskew needs %d images" % self.n_local)
        motion, keep = sweep_motion(self.n_local, knot_times, knot_poses, ref_times)
        ptrs = (ctypes.c_void_p * max(len(images), 1))(*[a.ctypes.data for a in images])
        counts = np.zeros(self.n_local, np.int32)
        rc = lib().locgpu_batch_upload_ranges_deskew(self._h, sensor._h, ptrs, ctypes.byref(motion), counts.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.counts = counts
            raise err
        return counts

    def _record_args(self, layout, blobs):
        L = point_layout(layout)
        blobs = [_records(L, x) for x in blobs]
        if len(blobs) != self.n_local:
            raise ValueError("a record upload needs %d blobs" % self.n_local)
        ptrs = (ctypes.c_void_p * max(len(blobs), 1))(*[(a.ctypes.data if n else None) for a, n in blobs])
        n_points = np.array([n for _, n in blobs], np.int64)
        return L, blobs, ptrs, n_points

    def upload_records(self, layout, blobs):
        """Replace the batch's scans by Conver's survivors of one blob of point records per scan (locgpu_batch_upload_records; ``layout``
        a dict such as LAYOUT_VELODYNE or a PointLayoutC) and leave their ring bytes resident when the layout has a ring field.
        Blocking. Returns the counts; when a scan does not fit the batch the LocGpuError carries the needed counts as ``.counts``."""
        self.upload_wait()
        L, keep, ptrs, n_points = self._record_args(layout, blobs)
        counts = np.zeros(self.n_local, np.int32)
        rc = lib().locgpu_batch_upload_records(self._h, ctypes.byref(L), ptrs, n_points.ctypes.data, counts.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.counts = counts
            raise err
        return counts

    def upload_records_deskew(self, layout, blobs, time_offsets, knot_times, knot_poses, ref_times):
        """upload_records with every survivor motion-compensated at its own time (locgpu_batch_upload_records_deskew): time_offsets [n]
        (a point's time is field * layout.time_scale + time_offsets[s]), knot_times [n, K], knot_poses [n, K, 7], ref_times [n]. A
        refused call raises a LocGpuError that carries ``.counts`` and ``.status`` (1 for a scan with a refused survivor time)."""
        self.upload_wait()
        L, keep, ptrs, n_points = self._record_args(layout, blobs)
        offs = np.ascontiguousarray(time_offsets, dtype=np.float64).reshape(-1)
        if len(offs) != self.n_local:
            raise ValueError("one time offset per scan")
        motion, keep_m = sweep_motion(self.n_local, knot_times, knot_poses, ref_times)
        counts, status = np.zeros(self.n_local, np.int32), np.zeros(self.n_local, np.int32)
        rc = lib().locgpu_batch_upload_records_deskew(self._h, ctypes.byref(L), ptrs, n_points.ctypes.data, offs.ctypes.data, ctypes.byref(motion), counts.ctypes.data,
                                                      status.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.counts, err.status = counts, status
            raise err
        return counts

    def download_rings(self, s):
        """The resident ring bytes of scan ``s`` (uint8, one per point); refused when the batch holds none."""
        self.upload_wait()
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_batch_download_rings(self._h, int(s), None, 0, ctypes.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        if n.value:
            self.ctx._check(lib().locgpu_batch_download_rings(self._h, int(s), out.ctypes.data, int(n.value), ctypes.byref(n)))
        return out

    def keep_times(self, on=True):
        """Make the plain ingest calls (upload_records, upload_ranges) leave one float64 time key per survivor beside the ring bytes
        (locgpu_batch_keep_times): what deskew needs. Off by default; off frees the times the batch holds."""
        self.ctx._check(lib().locgpu_batch_keep_times(self._h, int(bool(on))))

    def download_times(self, s):
        """The resident time keys of scan ``s`` (float64, one per point); refused when the batch holds none."""
        self.upload_wait()
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_batch_download_times(self._h, int(s), None, 0, ctypes.byref(n)))
        out = np.zeros(int(n.value), np.float64)
        if n.value:
            self.ctx._check(lib().locgpu_batch_download_times(self._h, int(s), out.ctypes.data, int(n.value), ctypes.byref(n)))
        return out

    def deskew(self, dst=None, time_offsets=None, *, knot_times, knot_poses, ref_times):
        """Motion-compensate the resident scans at their kept point times (locgpu_batch_deskew) into ``dst`` (None: in place): a point's
        time is its key + time_offsets[s] (None: the key alone); knot_times [n, K], knot_poses [n, K, 7], ref_times [n] as in
        upload_records_deskew, e.g. from motion_from_poses. The bytes are those of the deskewed ingest of the same scans. Blocking. A
        refused call raises a LocGpuError that carries ``.status`` (1 for a scan with a refused point time)."""
        self.upload_wait()
        dst = self if dst is None else dst
        dst.upload_wait()
        offs = None
        if time_offsets is not None:
            offs = np.ascontiguousarray(time_offsets, dtype=np.float64).reshape(-1)
            if len(offs) != self.n_local:
                raise ValueError("one time offset per scan")
        motion, keep_m = sweep_motion(self.n_local, knot_times, knot_poses, ref_times)
        status = np.zeros(self.n_local, np.int32)
        rc = lib().locgpu_batch_deskew(self._h, dst._h, offs.ctypes.data if offs is not None else None, ctypes.byref(motion), status.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.status = status
            raise err
        return dst

    def loam_extract_resident(self, num_scan, edge, surf):
        """loam_extract with the ring bytes upload_ranges left in the batch (locgpu_batch_loam_extract_resident); same returns and errors."""
        self.upload_wait()
        edge.upload_wait()
        surf.upload_wait()
        ne, ns, status = (np.zeros(self.n_local, np.int32) for _ in range(3))
        rc = lib().locgpu_batch_loam_extract_resident(self._h, int(num_scan), edge._h, surf._h, ne.ctypes.data, ns.ctypes.data, status.ctypes.data)
        if rc != 0:
            err = LocGpuError(rc, lib().locgpu_last_error(self.ctx._h).decode())
            err.edge_counts, err.surf_counts, err.status = ne, ns, status
            raise err
        return ne, ns, status

    def upload_clouds(self, clouds):
        """Fill the batch's scans from resident clouds (device-to-device, {x, y, z, 0}); clouds of other contexts on the GPU are accepted."""
        self.upload_wait()
        clouds = list(clouds)
        arr = (ctypes.c_void_p * max(len(clouds), 1))(*[c._h for c in clouds])
        self.ctx._check(lib().locgpu_batch_upload_clouds(self._h, arr, len(clouds)))

    def merge(self, poses, leaf, use=None, out=None, with_passthrough=False):
        """The scans of the batch as one map (locgpu_batch_merge): scan s under ``poses[s]`` ([n_scans, 7], or None), joined in scan
        order, one voxel filter (``leaf`` 0: join only). ``use`` (n_scans booleans or None): scans to leave out. Equals
        Context.clouds_merge of the clouds export_cloud makes; the batch is not modified."""
        self.upload_wait()
        p = _pose(poses).reshape(self.n_local, 7) if poses is not None else None
        u = None
        if use is not None:
            u = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
            if u.shape != (self.n_local,):
                raise ValueError("use needs %d entries" % self.n_local)
        out = out if out is not None else Cloud(self.ctx)
        pt = ctypes.c_int(0)
        self.ctx._check(lib().locgpu_batch_merge(self._h, p.ctypes.data if p is not None else None, u.ctypes.data if u is not None else None, float(leaf),
                                                 out._h, ctypes.byref(pt)))
        return (out, bool(pt.value)) if with_passthrough else out

    def export_cloud(self, scan, cloud=None):
        """Scan ``scan`` as a resident cloud {x, y, z, 0}, not flagged dense (locgpu_batch_export_cloud); ``cloud`` may belong to any
        context on the GPU (None = a new cloud of the batch's context)."""
        self.upload_wait()
        cloud = cloud if cloud is not None else Cloud(self.ctx)
        self.ctx._check(lib().locgpu_batch_export_cloud(self._h, int(scan), cloud._h))
        return cloud

    def download_scan(self, s):
        """Scan ``s`` of the batch as an [n, 4] float32 array: x, y, z and the fourth lane as the batch holds it."""
        self.upload_wait()
        n = ctypes.c_size_t(0)
        self.ctx._check(lib().locgpu_batch_download_scan(self._h, int(s), None, 0, 16, ctypes.byref(n)))
        out = np.zeros((int(n.value), 4), np.float32)
        if n.value:
            self.ctx._check(lib().locgpu_batch_download_scan(self._h, int(s), out.ctypes.data, int(n.value), 16, ctypes.byref(n)))
        return out

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().locgpu_batch_destroy(self._h)
        self._h = None
        self._keep = None

    def __del__(self):
        self.close()


class Pool:
    """The open-scan pool (locgpu_pool): jobs of scans submitted at any time, iterated together, collected by ticket."""

    def __init__(self, ctx, slots, max_points, scans_per_job=0, chunk=0, opts=None, ndt=False, prefetch=-1):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        self._keep, self._n = {}, {}
        o = PoolOpts()
        lib().locgpu_pool_opts_default(ctypes.byref(o))
        o.slots, o.scans_per_job, o.chunk, o.matcher, o.max_points = int(slots), int(scans_per_job), int(chunk), (1 if ndt else 0), int(max_points)
        o.prefetch = int(prefetch)
        if opts is not None:
            o.icp = opts
        ctx._check(lib().locgpu_pool_create(ctx._h, ctypes.byref(o), ctypes.byref(self._h)))

    def submit(self, scans, init_poses, first=0, n_total=None):
        """scans: the scans this rank holds of the job (a list or MarshalledScans; may be empty on a rank of a sharded job);
        init_poses: [n_total, 7]. Returns the ticket."""
        n_total = len(scans) if n_total is None else int(n_total)
        ip = _pose(init_poses).reshape(n_total, 7)
        t = ctypes.c_int64(0)
        if len(scans):
            sc, ptrs, cnts, stride = Batch._marshal(scans)
        else:
            sc, ptrs, cnts, stride = [], None, None, 16
        rc = lib().locgpu_pool_submit(self._h, ptrs, cnts, stride, len(sc), int(first), n_total, ip.ctypes.data, ctypes.byref(t))
        if t.value:  # the job was accepted (a ticket was handed out): whatever rc says, the upload service may be reading the clouds
            self._keep[t.value] = (sc, ptrs, cnts)  # they stay alive until the ticket has been waited for
            self._n[t.value] = n_total
        self.ctx._check(rc)
        return t.value

    def wait(self, ticket):
        n = self._n.pop(ticket, None)
        if n is None:
            raise LocGpuError(-1, "pool.wait: unknown ticket (a ticket is good once)")
        out = np.zeros((n, 7))
        st = (AlignStats * n)()
        rc = lib().locgpu_pool_wait(self._h, ctypes.c_int64(ticket), out.ctypes.data, st)
        self._keep.pop(ticket, None)
        self.ctx._check(rc)
        return out, [_stats_dict(s) for s in st]

    def step(self, block=True):
        """One turn of the pool (look at the chunk in flight, scans out, jobs in, next chunk) without collecting a job."""
        self.ctx._check(lib().locgpu_pool_step(self._h, 1 if block else 0))

    def done(self, ticket):
        d = ctypes.c_int(0)
        self.ctx._check(lib().locgpu_pool_done(self._h, ctypes.c_int64(ticket), ctypes.byref(d)))
        return bool(d.value)

    def info(self):
        out = (ctypes.c_int64 * 8)()
        self.ctx._check(lib().locgpu_pool_info(self._h, out))
        return dict(slots=out[0], free=out[1], jobs=out[2], iterations=out[3], scan_iterations=out[4], open=out[5], regions=out[6], free_regions=out[7])

    def profile_read(self, reset=True):
        out = (ctypes.c_double * 2)()
        self.ctx._check(lib().locgpu_pool_profile_read(self._h, out, 1 if reset else 0))
        return dict(chunk_ms=out[0], chunks=int(out[1]))

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().locgpu_pool_destroy(self._h)
        self._h = None
        self._keep = {}

    def __del__(self):
        self.close()


class Loam:
    """One LoamRegistration on one GPU (locgpu_loam): an edge matcher (P2Line) and a surface matcher (P2Plane) whose joint
    Gauss–Newton loop runs on the device (loam_registration.cpp:22-99). A feature class that is switched off takes None."""

    def __init__(self, opts=None, device_id=0):
        self._h = ctypes.c_void_p()
        self.opts = opts if opts is not None else loam_opts()
        rc = lib().locgpu_loam_create(device_id, ctypes.byref(self.opts), ctypes.byref(self._h))
        if rc != 0:
            raise LocGpuError(rc, lib().locgpu_loam_last_error(None).decode())

    @classmethod
    def on(cls, surf_ctx, edge_ctx, opts=None):
        """The matcher over two existing Contexts (locgpu_loam_create_on): their targets are borrowed, and they outlive the handle.
        None for the context of a class that is switched off."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.opts = opts if opts is not None else loam_opts()
        self._ctxs = (surf_ctx, edge_ctx)  # kept alive: the handle must go first
        rc = lib().locgpu_loam_create_on(surf_ctx._h if surf_ctx is not None else None, edge_ctx._h if edge_ctx is not None else None,
                                         ctypes.byref(self.opts), ctypes.byref(self._h))
        if rc != 0:
            raise LocGpuError(rc, lib().locgpu_loam_last_error(None).decode())
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().locgpu_loam_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise LocGpuError(rc, lib().locgpu_loam_last_error(self._h).decode())

    @staticmethod
    def _arg(cloud):
        """(array kept alive, pointer, count, stride) of an optional cloud"""
        if cloud is None:
            return None, None, 0, 0
        c = _cloud(cloud)
        return c, c.ctypes.data, c.shape[0], c.strides[0]

    @staticmethod
    def _stride(se, ss):
        if se and ss and se != ss:
            raise ValueError("edge and surface clouds must share one point stride")
        return se or ss or 12

    # ---- LoamRegistration::SetInputTarget
    def set_target(self, edge_map, surf_map):
        e, pe, ne, se = self._arg(edge_map)
        s, ps, ns, ss = self._arg(surf_map)
        self._check(lib().locgpu_loam_set_target(self._h, pe, ne, ps, ns, self._stride(se, ss)))

    # ---- one evaluation of H_surf + H_edge, B_surf + B_edge; eff / ok per class, index 0 = surface, 1 = edge
    def hb(self, edge, surf, pose):
        e, pe, ne, se = self._arg(edge)
        s, ps, ns, ss = self._arg(surf)
        H, B = np.zeros(36), np.zeros(6)
        eff, ok = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
        self._check(lib().locgpu_loam_hb(self._h, pe, ne, ps, ns, self._stride(se, ss), _pose(pose).ctypes.data, H.ctypes.data, B.ctypes.data,
                                         eff.ctypes.data, ok.ctypes.data))
        return H.reshape(6, 6), B, [int(v) for v in eff], [bool(v) for v in ok]

    # ---- LoamRegistration::ScanMatch whole; result_pose in-out (status 3 / 4 leaves it, and the output cloud, as handed in)
    def scan_match(self, edge, surf, init_pose, result_pose=None, out_cloud=None):
        """Returns (pose, stats, output cloud [n_edge + n_surf, 3] float32: edge points, then surface points)."""
        e, pe, ne, se = self._arg(edge)
        s, ps, ns, ss = self._arg(surf)
        cloud = out_cloud if out_cloud is not None else np.full((ne + ns, 3), np.nan, np.float32)
        out = np.array(_pose(result_pose if result_pose is not None else init_pose), copy=True)
        st = AlignStats()
        self._check(lib().locgpu_loam_scan_match(self._h, pe, ne, ps, ns, self._stride(se, ss), _pose(init_pose).ctypes.data, out.ctypes.data,
                                                 ctypes.byref(st), cloud.ctypes.data if cloud.size else None, cloud.strides[0]))
        return out, _stats_dict(st), cloud

    # ---- the same on resident clouds (api.Cloud of any Context on this GPU; None for a class that is switched off)
    def set_target_cloud(self, edge_map, surf_map, wait=True):
        """wait=False: returns once both clouds are copied out; the host tree builds run on worker threads and the next call that
        reads the target completes the ingest."""
        fn = lib().locgpu_loam_set_target_cloud if wait else lib().locgpu_loam_set_target_cloud_async
        self._check(fn(self._h, edge_map._h if edge_map is not None else None, surf_map._h if surf_map is not None else None))

    def scan_match_cloud(self, edge, surf, init_pose, result_pose=None, out=None):
        """Returns (pose, stats). out (an api.Cloud distinct from edge and surf, optional) receives the edge points, then the surface
        points, under the result; status 3 / 4 leaves it, and result_pose, as handed in."""
        pose = np.array(_pose(result_pose if result_pose is not None else init_pose), copy=True)
        st = AlignStats()
        self._check(lib().locgpu_loam_scan_match_cloud(self._h, edge._h if edge is not None else None, surf._h if surf is not None else None,
                                                       _pose(init_pose).ctypes.data, pose.ctypes.data, ctypes.byref(st), out._h if out is not None else None))
        return pose, _stats_dict(st)

    def fitness_resident(self, pose, max_range=1.0):
        """[surface, edge] scores (dicts as Context.icp_fitness) of the scans the last single-scan call left in HBM; after
        scan_match_cloud those are the caller's clouds, which must still be alive and unmodified."""
        out = (Fitness * 2)()
        self._check(lib().locgpu_loam_fitness_resident(self._h, _pose(pose).ctypes.data, float(max_range), out))
        return [_fitness_dict(out[0]), _fitness_dict(out[1])]

    # ---- the joint score and the initial-pose search: one pair of scans under many poses. Three entries per pose: joint, surface, edge
    @staticmethod
    def _fit3(fit, m, raw):
        return fit if raw else [[_fitness_dict(fit[3 * i + j]) for j in range(3)] for i in range(m)]

    def fitness(self, edge, surf, poses, max_range=1.0, raw=False):
        """Per pose [joint, surface, edge] (dicts as Context.icp_fitness; raw=True: the ctypes array of 3 entries per pose)."""
        e, pe, ne, se = self._arg(edge)
        s, ps, ns, ss = self._arg(surf)
        p = _pose(poses).reshape(-1, 7)
        out = (Fitness * (3 * max(len(p), 1)))()
        self._check(lib().locgpu_loam_fitness(self._h, pe, ne, ps, ns, self._stride(se, ss), p.ctypes.data, len(p), float(max_range), out))
        return self._fit3(out, len(p), raw)

    def fitness_cloud(self, edge, surf, poses, max_range=1.0, raw=False):
        p = _pose(poses).reshape(-1, 7)
        out = (Fitness * (3 * max(len(p), 1)))()
        self._check(lib().locgpu_loam_fitness_cloud(self._h, edge._h if edge is not None else None, surf._h if surf is not None else None, p.ctypes.data,
                                                    len(p), float(max_range), out))
        return self._fit3(out, len(p), raw)

    def _search(self, call, head, candidates, sopts, raw):
        c = _pose(candidates).reshape(-1, 7)
        m = c.shape[0]
        out = np.zeros((m, 7))
        fit = (Fitness * (3 * max(m, 1)))()
        st = (AlignStats * max(m, 1))()
        best = ctypes.c_int(-2)
        self._check(call(self._h, *head, c.ctypes.data, m, ctypes.byref(sopts) if sopts is not None else None, out.ctypes.data, fit, st, ctypes.byref(best)))
        return out, self._fit3(fit, m, raw), [_stats_dict(x) for x in st], int(best.value)

    def init_search(self, edge, surf, candidates, sopts=None, raw=False):
        """Returns (poses [m, 7], per candidate [joint, surface, edge] fitness, stats, best index by the joint score or -1)."""
        e, pe, ne, se = self._arg(edge)
        s, ps, ns, ss = self._arg(surf)
        return self._search(lib().locgpu_loam_init_search, (pe, ne, ps, ns, self._stride(se, ss)), candidates, sopts, raw)

    def init_search_cloud(self, edge, surf, candidates, sopts=None, raw=False):
        return self._search(lib().locgpu_loam_init_search_cloud, (edge._h if edge is not None else None, surf._h if surf is not None else None), candidates, sopts, raw)

    # ---- many feature scans against the one pair of maps
    def align_batch(self, edges, surfs, init_poses):
        """edges / surfs: lists of clouds (None for a class that is switched off). Returns (poses [n, 7], list of stats)."""
        n = len(edges) if edges is not None else len(surfs)
        me = Batch._marshal(edges) if edges is not None else (None, None, None, 0)
        ms = Batch._marshal(surfs) if surfs is not None else (None, None, None, 0)
        poses = _pose(init_poses).reshape(n, 7)
        out = np.zeros((n, 7))
        st = (AlignStats * n)()
        self._check(lib().locgpu_loam_align_batch(self._h, n, me[1], me[2], ms[1], ms[2], self._stride(me[3], ms[3]), poses.ctypes.data, out.ctypes.data, st))
        return out, [_stats_dict(x) for x in st]


    def align_batches(self, edge, surf, init_poses):
        """align_batch on two resident batches (api.Batch of any Context on this GPU; None for a class that is switched off): scan i
        of ``edge`` with scan i of ``surf``. Returns (poses [n, 7], list of stats), the bits of align_batch on the downloaded scans."""
        some = edge if edge is not None else surf
        n = some.n_local
        for b in (edge, surf):
            if b is not None:
                b.upload_wait()
        poses = _pose(init_poses).reshape(n, 7)
        out = np.zeros((n, 7))
        st = (AlignStats * max(n, 1))()
        self._check(lib().locgpu_loam_align_batches(self._h, edge._h if edge is not None else None, surf._h if surf is not None else None, poses.ctypes.data,
                                                    out.ctypes.data, st))
        return out, [_stats_dict(st[i]) for i in range(n)]


def gn_update(hb, method, min_effective_pts, eps, pose):
    """Host-side Gauss–Newton update on reduced normal equations (point-sharded multi-GPU mode)."""
    hb = np.ascontiguousarray(hb, dtype=np.float64).reshape(44)
    p = np.array(_pose(pose), copy=True)
    dx = np.zeros(6)
    applied, stop = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().locgpu_gn_update(hb.ctypes.data, method, min_effective_pts, eps, p.ctypes.data, dx.ctypes.data, ctypes.byref(applied),
                                ctypes.byref(stop))
    if rc != 0:
        raise LocGpuError(rc, "gn_update failed")
    return p, dx, bool(applied.value), bool(stop.value)
