"""ctypes binding of libfgoicp_amd.so (include/fgoicp_amd.h).  Loading fails loudly when the
library has not been built; there is no Python or CPU fallback for any operator."""
import ctypes as C
import os

from . import build as _build

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_uint32_p = C.POINTER(C.c_uint32)
c_uint8_p = C.POINTER(C.c_uint8)
c_double_p = C.POINTER(C.c_double)


class CtxInfo(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("lut_dims", C.c_int * 3), ("lut_layout", C.c_int), ("lut_nodes", C.c_uint64), ("lut_bytes", C.c_uint64),
                ("source_points_per_face_voxel", C.c_double), ("points_per_item", C.c_int), ("items_per_evaluation", C.c_int),
                ("max_subcubes_per_window", C.c_int), ("source_order", C.c_int), ("tree_order", C.c_int), ("chunks_per_item_with_thresholds", C.c_int)]


class CloudStats(C.Structure):
    _fields_ = [("n", C.c_uint64), ("centroid", C.c_float * 3), ("min", C.c_float * 3), ("max", C.c_float * 3), ("max_abs_centred", C.c_float),
                ("rms_radius", C.c_float)]


class Exchange(C.Structure):
    ALLREDUCE_MIN = C.CFUNCTYPE(C.c_int, c_float_p, C.c_size_t, C.c_void_p)
    ALLGATHER = C.CFUNCTYPE(C.c_int, c_float_p, c_float_p, C.c_size_t, C.c_void_p)
    ALLGATHER_DEVICE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
    _fields_ = [("struct_size", C.c_size_t), ("rank", C.c_int), ("world_size", C.c_int), ("allreduce_min", ALLREDUCE_MIN),
                ("allgather", ALLGATHER), ("user", C.c_void_p), ("allgather_device", ALLGATHER_DEVICE)]  # the last one optional (NULL: no cooperative ICP)

    def __init__(self, rank=0, world_size=1, allreduce_min=None, allgather=None, user=None, allgather_device=None):
        super().__init__()
        self.struct_size = C.sizeof(Exchange)  # ABI 2: the library reads no byte beyond it
        self.rank, self.world_size, self.user = rank, world_size, user
        if allreduce_min is not None:
            self.allreduce_min = allreduce_min
        if allgather is not None:
            self.allgather = allgather
        if allgather_device is not None:
            self.allgather_device = allgather_device


class SolverOpts(C.Structure):
    _fields_ = [("schedule", C.c_int), ("round_width", C.c_int), ("ctx_flags", C.c_uint), ("device", C.c_int), ("trim_fraction", C.c_float)]


class RunStats(C.Structure):
    _fields_ = [("trans_cubes", C.c_uint64), ("bounds_calls", C.c_uint64), ("rot_cubes", C.c_uint64),
                ("icp_runs", C.c_uint64), ("icp_iters", C.c_uint64), ("inner_bnb", C.c_uint64),
                ("rounds", C.c_uint64), ("seconds_total", C.c_double), ("seconds_bnb", C.c_double),
                ("seconds_icp", C.c_double), ("initial_icp_sse", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FLAG_NO_WEIGHT_QUANT = 1 << 0
FLAG_NO_MORTON = 1 << 1
FLAG_PROFILE = 1 << 2
FLAG_BRUTE_FORCE_NN = 1 << 3
FLAG_CURVE_ORDER = 1 << 4
class BatchPair(C.Structure):
    _fields_ = [("tgt_xyz", c_float_p), ("nt", C.c_size_t), ("src_xyz", c_float_p), ("ns", C.c_size_t), ("lut_resolution", C.c_float),
                ("mse_threshold", C.c_float)]


class BatchOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("solver", SolverOpts), ("max_live", C.c_int), ("trim_fractions", c_float_p),  # n entries or NULL
                ("alignment", C.c_int)]  # != 0: the run keeps every pair's alignment report (fgoicp_batch_alignment)


class BatchOptsInformation(BatchOpts):
    """fgoicp_batch_opts whole: BatchOpts is the struct as first published with `alignment` (48 bytes, still accepted: struct_size); the members
    appended since start behind its tail padding (reserved0 in the header)."""
    _fields_ = [("information", C.c_int),  # != 0: the run keeps every pair's information matrix (fgoicp_batch_information)
                ("information_max_distance", C.c_float)]  # callers' units; <= 0: no threshold


class BatchRefine(C.Structure):
    """fgoicp_batch_refine_t: how one pair of a batch is refined after its search; model = -1: not at all."""
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_int), ("k", C.c_int), ("max_iter", C.c_size_t), ("conv_thr", C.c_float), ("max_distance", C.c_float),
                ("epsilon", C.c_double), ("loss", C.c_int), ("loss_scale", C.c_double)]


class BatchOptsRefine(BatchOptsInformation):
    """fgoicp_batch_opts_refine: fgoicp_batch_opts (56 bytes, as published) followed by the refine table (n entries or NULL)."""
    _fields_ = [("refine", C.POINTER(BatchRefine))]


class AlignmentSummary(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("inliers", C.c_uint64), ("targets_hit", C.c_uint64), ("sse", C.c_float),
                ("max_inlier_dist2", C.c_float), ("scaling_factor", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(AlignmentSummary)  # the library writes no byte beyond it


class Information(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("correspondences", C.c_uint64), ("sum_dist2", C.c_double), ("sum_q", C.c_double * 3),
                ("sum_qq", C.c_double * 6), ("info", C.c_double * 36), ("max_dist2", C.c_float), ("scaling_factor", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(Information)  # the library writes no byte beyond it


class PlaneMoments(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("correspondences", C.c_uint64), ("m", C.c_double * 28), ("max_dist2", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(PlaneMoments)  # the library writes no byte beyond it


class PlaneResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("iterations", C.c_int), ("rank", C.c_int), ("correspondences", C.c_uint64),
                ("plane_rmse", C.c_double), ("sse", C.c_float), ("scaling_factor", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(PlaneResult)  # the library writes no byte beyond it


class RobustMoments(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("correspondences", C.c_uint64), ("m", C.c_double * 28), ("weight_sum", C.c_double),
                ("max_dist2", C.c_float), ("loss", C.c_int), ("scale", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(RobustMoments)  # the library writes no byte beyond it


class RobustResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("iterations", C.c_int), ("rank", C.c_int), ("correspondences", C.c_uint64),
                ("weight_sum", C.c_double), ("rmse", C.c_double), ("sse", C.c_float), ("scaling_factor", C.c_float), ("loss", C.c_int), ("scale_estimated", C.c_int),
                ("scale", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(RobustResult)  # the library writes no byte beyond it


LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY, LOSS_GEMAN_MCCLURE, LOSS_TUKEY = range(5)
LOSSES = {"none": LOSS_NONE, "huber": LOSS_HUBER, "cauchy": LOSS_CAUCHY, "geman_mcclure": LOSS_GEMAN_MCCLURE, "tukey": LOSS_TUKEY}
MODEL_PLANE, MODEL_GICP = 0, 1


class VoxelInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("voxels", C.c_uint64), ("max_points_per_voxel", C.c_uint64), ("origin", C.c_float * 3),
                ("voxel_size", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(VoxelInfo)  # the library writes no byte beyond it


class OutlierInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("kept", C.c_uint64), ("mode", C.c_int), ("k", C.c_int), ("mean", C.c_double),
                ("stddev", C.c_double), ("threshold", C.c_double), ("radius2", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(OutlierInfo)  # the library writes no byte beyond it


class FpsInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("samples", C.c_uint64), ("start_index", C.c_uint64), ("next_index", C.c_uint64),
                ("cover_dist2", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(FpsInfo)  # the library writes no byte beyond it


class ClusterInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("core_points", C.c_uint64), ("border_points", C.c_uint64), ("noise_points", C.c_uint64),
                ("clusters", C.c_uint64), ("largest_label", C.c_int64), ("largest_size", C.c_uint64), ("kept", C.c_uint64), ("keep_min_size", C.c_uint64),
                ("min_points", C.c_int), ("eps2", C.c_float), ("rounds", C.c_uint32)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(ClusterInfo)  # the library writes no byte beyond it


class SegmentModel(C.Structure):
    _fields_ = [("candidates", C.c_uint64), ("sample", C.c_uint32 * 3), ("hypothesis", C.c_uint32), ("hypothesis_inliers", C.c_uint64), ("inliers", C.c_uint64),
                ("hypothesis_plane", C.c_double * 4), ("plane", C.c_double * 4), ("pivot", C.c_double * 3), ("sum_u", C.c_double * 3), ("sum_uu", C.c_double * 6)]


class SegmentInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("points", C.c_uint64), ("planes", C.c_uint64), ("on_planes", C.c_uint64), ("kept", C.c_uint64), ("iterations", C.c_int),
                ("max_planes", C.c_int), ("refit", C.c_int), ("keep_planes", C.c_int), ("min_inliers", C.c_uint64), ("seed", C.c_uint64),
                ("distance_threshold", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(SegmentInfo)  # the library writes no byte beyond it


class MeshInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("vertices", C.c_uint64), ("triangles", C.c_uint64), ("samples", C.c_uint64), ("zero_area", C.c_uint64),
                ("unweighted", C.c_uint64), ("weight_total", C.c_uint64), ("max_area", C.c_double), ("area", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(MeshInfo)  # the library writes no byte beyond it


class MeshDistanceInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("vertices", C.c_uint64), ("triangles", C.c_uint64), ("queries", C.c_uint64), ("faces", C.c_uint64),
                ("zero_area", C.c_uint64), ("tree_depth", C.c_uint32), ("leaf_faces", C.c_uint32), ("max_dist2_index", C.c_uint64), ("max_dist2", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(MeshDistanceInfo)  # the library writes no byte beyond it


class MeshMoments(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("points", C.c_uint64), ("correspondences", C.c_uint64), ("m", C.c_double * 28), ("weight_sum", C.c_double),
                ("sum_dist2", C.c_double), ("max_dist2", C.c_double), ("loss", C.c_int), ("scale", C.c_double), ("vertices", C.c_uint64), ("triangles", C.c_uint64),
                ("faces", C.c_uint64), ("zero_area", C.c_uint64), ("tree_depth", C.c_uint32), ("leaf_faces", C.c_uint32)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(MeshMoments)  # the library writes no byte beyond it


class MeshRefineResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("iterations", C.c_int), ("rank", C.c_int), ("points", C.c_uint64),
                ("correspondences", C.c_uint64), ("weight_sum", C.c_double), ("mesh_rmse", C.c_double), ("rms_distance", C.c_double), ("loss", C.c_int),
                ("scale_estimated", C.c_int), ("loss_scale", C.c_double), ("triangles", C.c_uint64), ("faces", C.c_uint64), ("zero_area", C.c_uint64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(MeshRefineResult)  # the library writes no byte beyond it


MESH_DISTANCE_BRUTE = 1

OUTLIER_STATISTICAL = 0
OUTLIER_RADIUS = 1

SCHEDULE_SERIAL = 0
SCHEDULE_ROUND = 1

_SIGS = {
    "fgoicp_last_error": (C.c_char_p, []),
    "fgoicp_version": (C.c_char_p, []),
    "fgoicp_dev_knobs": (C.c_int, []),
    "fgoicp_abi_version": (C.c_int, []),
    "fgoicp_ctx_create": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, C.c_float, C.c_int, C.c_uint,
                                    C.POINTER(C.c_void_p)]),
    "fgoicp_ctx_destroy": (None, [C.c_void_p]),
    "fgoicp_lut_dims": (C.c_int, [C.c_void_p, c_int_p]),
    "fgoicp_ctx_get_info": (C.c_int, [C.c_void_p, C.POINTER(CtxInfo)]),
    "fgoicp_cloud_stats": (C.c_int, [c_float_p, C.c_size_t, C.POINTER(CloudStats)]),
    "fgoicp_voxel_downsample": (C.c_int, [c_float_p, C.c_size_t, C.c_float, c_float_p, C.c_int, c_float_p, C.c_size_t, c_uint32_p, c_uint32_p, C.POINTER(VoxelInfo)]),
    "fgoicp_remove_outliers": (C.c_int, [c_float_p, C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_int, c_float_p, C.c_size_t, c_uint32_p, c_uint8_p, c_double_p, c_float_p,
                                         C.POINTER(OutlierInfo)]),
    "fgoicp_farthest_point_sample": (C.c_int, [c_float_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, c_float_p, c_uint32_p, c_float_p, c_float_p, c_uint32_p,
                                               C.POINTER(FpsInfo)]),
    "fgoicp_cluster_dbscan": (C.c_int, [c_float_p, C.c_size_t, C.c_float, C.c_int, C.c_size_t, C.c_int, c_float_p, C.c_size_t, c_uint32_p, C.POINTER(C.c_int32), c_uint32_p,
                                        C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(ClusterInfo)]),
    "fgoicp_segment_planes": (C.c_int, [c_float_p, C.c_size_t, C.c_float, C.c_int, C.c_uint64, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, c_float_p, C.c_size_t,
                                        c_uint32_p, C.POINTER(C.c_int32), C.POINTER(SegmentModel), C.c_size_t, C.c_size_t, C.POINTER(SegmentInfo)]),
    "fgoicp_segment_hypotheses": (C.c_int, [c_float_p, C.c_size_t, c_uint32_p, C.c_size_t, C.c_int, C.c_uint64, C.c_int, c_uint32_p, C.POINTER(C.c_double), c_uint8_p]),
    "fgoicp_segment_fit_from_moments": (C.c_int, [C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double)]),
    "fgoicp_mesh_sample": (C.c_int, [c_float_p, C.c_size_t, c_uint32_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_int, c_float_p, c_float_p, c_uint32_p, c_double_p, c_double_p,
                                     C.POINTER(MeshInfo)]),
    "fgoicp_mesh_distance": (C.c_int, [c_float_p, C.c_size_t, c_uint32_p, C.c_size_t, c_float_p, C.c_size_t, C.c_uint32, C.c_int, c_uint32_p, c_float_p, c_double_p, c_uint8_p,
                                       C.POINTER(C.c_int8), C.POINTER(MeshDistanceInfo)]),
    "fgoicp_point_triangle": (C.c_int, [c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, C.POINTER(C.c_double), c_int_p, c_int_p]),
    "fgoicp_mesh_pair_terms": (C.c_int, [c_float_p, c_float_p, c_float_p, c_float_p, C.c_int, C.c_double, c_double_p, c_double_p, c_int_p, c_double_p, c_double_p, c_double_p,
                                         c_double_p]),
    "fgoicp_mesh_moments": (C.c_int, [c_float_p, C.c_size_t, c_uint32_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, c_float_p, C.c_float, C.c_int, C.c_double, C.c_uint32,
                                      C.c_int, c_uint32_p, c_float_p, c_double_p, c_uint8_p, c_double_p, c_double_p, c_double_p, c_uint8_p, c_uint32_p, C.POINTER(MeshMoments)]),
    "fgoicp_mesh_refine": (C.c_int, [c_float_p, C.c_size_t, c_uint32_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, c_float_p, C.c_size_t, C.c_float, C.c_float, C.c_int,
                                     C.c_double, C.c_uint32, C.c_int, C.POINTER(MeshRefineResult)]),
    "fgoicp_solver_set_target_normals": (C.c_int, [C.c_void_p, c_float_p]),
    "fgoicp_solver_set_source_normals": (C.c_int, [C.c_void_p, c_float_p]),
    "fgoicp_lut_read": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t]),
    "fgoicp_lut_search": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_float_p]),
    "fgoicp_lut_nodes": (C.c_int, [C.c_void_p, c_int_p, C.c_size_t, c_float_p]),
    "fgoicp_bounds_point_distances": (C.c_int, [C.c_void_p, c_float_p, C.c_float, c_float_p, C.c_int, c_float_p]),
    "fgoicp_ctx_sort_fallbacks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fgoicp_ctx_test_sort_fault": (C.c_int, [C.c_void_p, C.c_int]),
    "fgoicp_test_live_resources": (C.c_int, [C.POINTER(C.c_uint64)]),
    "fgoicp_bounds_batch": (C.c_int, [C.c_void_p, c_float_p, C.c_float, c_float_p, C.c_int, C.c_int, c_float_p, c_float_p]),
    "fgoicp_bounds_multi": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p, c_float_p,
                                      c_float_p]),
    "fgoicp_bounds_submit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p]),
    "fgoicp_bounds_submit_twins": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p, c_int_p]),
    "fgoicp_bounds_submit_cut": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p, c_int_p, c_float_p]),
    "fgoicp_bounds_submit_leaf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p, c_int_p, c_float_p, c_float_p]),
    "fgoicp_ctx_cut_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "fgoicp_solver_set_early_exit": (C.c_int, [C.c_void_p, C.c_int]),
    "fgoicp_bounds_collect": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p]),
    "fgoicp_sse": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p]),
    "fgoicp_alignment": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_uint32_p, c_float_p, c_uint8_p, c_uint8_p, C.POINTER(AlignmentSummary)]),
    "fgoicp_solver_alignment": (C.c_int, [C.c_void_p, c_uint32_p, c_float_p, c_uint8_p, c_uint8_p, C.POINTER(AlignmentSummary)]),
    "fgoicp_batch_alignment": (C.c_int, [C.c_void_p, C.c_int, c_uint32_p, c_float_p, c_uint8_p, c_uint8_p, C.POINTER(AlignmentSummary)]),
    "fgoicp_information": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_float, C.POINTER(Information)]),
    "fgoicp_solver_information": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(Information)]),
    "fgoicp_batch_information": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Information)]),
    "fgoicp_information_from_moments": (C.c_int, [C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), c_float_p, C.c_float, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fgoicp_ctx_set_target_normals": (C.c_int, [C.c_void_p, c_float_p, C.c_int]),
    "fgoicp_target_normals": (C.c_int, [C.c_void_p, c_float_p]),
    "fgoicp_target_knn": (C.c_int, [C.c_void_p, C.c_int, c_uint32_p, c_float_p]),
    "fgoicp_plane_moments": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_float, C.POINTER(PlaneMoments)]),
    "fgoicp_plane_step_from_moments": (C.c_int, [C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), c_int_p]),
    "fgoicp_plane_apply_step": (C.c_int, [c_float_p, c_float_p, C.POINTER(C.c_double), c_float_p, c_float_p]),
    "fgoicp_icp_plane": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t, C.c_float, C.c_float, C.POINTER(PlaneResult)]),
    "fgoicp_solver_refine_plane": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_float, C.POINTER(PlaneResult)]),
    "fgoicp_ctx_set_source_normals": (C.c_int, [C.c_void_p, c_float_p, C.c_int]),
    "fgoicp_source_normals": (C.c_int, [C.c_void_p, c_float_p]),
    "fgoicp_gicp_moments": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_float, C.c_double, C.POINTER(PlaneMoments)]),
    "fgoicp_icp_gicp": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t, C.c_float, C.c_float, C.c_double, C.POINTER(PlaneResult)]),
    "fgoicp_solver_refine_gicp": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_float, C.c_double, C.POINTER(PlaneResult)]),
    "fgoicp_gicp_terms": (C.c_int, [c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fgoicp_robust_weight": (C.c_int, [C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "fgoicp_robust_moments": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_float, C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(RobustMoments)]),
    "fgoicp_robust_residuals": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_float, C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), c_uint8_p]),
    "fgoicp_robust_scale": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_float, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "fgoicp_icp_robust": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(RobustResult)]),
    "fgoicp_solver_refine_robust": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_float, C.c_float, C.c_double, C.c_int, C.c_double, C.POINTER(RobustResult)]),
    "fgoicp_icp": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t, C.c_float, c_float_p, c_float_p, c_float_p, c_int_p]),
    "fgoicp_icp_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, C.c_size_t, C.c_float, c_float_p, c_float_p, c_float_p, c_int_p]),
    "fgoicp_procrustes": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int_p]),
    "fgoicp_ctx_set_inliers": (C.c_int, [C.c_void_p, C.c_size_t]),
    "fgoicp_ctx_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "fgoicp_ctx_profile_evaluations": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "fgoicp_ctx_profile_select_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fgoicp_ctx_trim_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "fgoicp_ctx_set_coop_split": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t]),
    "fgoicp_ctx_set_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "fgoicp_ctx_ns": (C.c_size_t, [C.c_void_p]),
    "fgoicp_ctx_nt": (C.c_size_t, [C.c_void_p]),
    "fgoicp_solver_create": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_float, C.c_float,
                                       C.POINTER(SolverOpts), C.POINTER(C.c_void_p)]),
    "fgoicp_solver_destroy": (None, [C.c_void_p]),
    "fgoicp_solver_set_exchange": (C.c_int, [C.c_void_p, C.POINTER(Exchange)]),
    "fgoicp_solver_set_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fgoicp_solver_run": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "fgoicp_solver_best_error": (C.c_int, [C.c_void_p, c_float_p]),
    "fgoicp_solver_best_transform": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "fgoicp_solver_last_transform": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "fgoicp_solver_stats": (C.c_int, [C.c_void_p, C.POINTER(RunStats)]),
    "fgoicp_solver_preproc": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p]),
    "fgoicp_solver_ctx": (C.c_void_p, [C.c_void_p]),
    "fgoicp_rccl_library": (C.c_char_p, []),
    "fgoicp_rccl_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "fgoicp_rccl_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.POINTER(C.c_void_p)]),
    "fgoicp_rccl_create_ex": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "fgoicp_rccl_test_inprogress": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "fgoicp_rccl_exchange": (C.c_int, [C.c_void_p, C.POINTER(Exchange)]),
    "fgoicp_rccl_calls": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "fgoicp_rccl_abort": (C.c_int, [C.c_void_p]),
    "fgoicp_rccl_comm_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "fgoicp_rccl_destroy": (None, [C.c_void_p]),
    "fgoicp_multi_create": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_float, C.c_float, C.POINTER(SolverOpts), c_int_p, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "fgoicp_multi_destroy": (None, [C.c_void_p]),
    "fgoicp_multi_run": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "fgoicp_multi_icp": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t, C.c_float, c_float_p, c_float_p, c_float_p, c_int_p]),
    "fgoicp_multi_world": (C.c_int, [C.c_void_p]),
    "fgoicp_multi_solver": (C.c_void_p, [C.c_void_p, C.c_int]),
    "fgoicp_multi_seconds": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "fgoicp_multi_set_record": (C.c_int, [C.c_void_p, C.c_int]),
    "fgoicp_multi_recorded": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fgoicp_multi_test_fault": (C.c_int, [C.c_void_p, C.c_int, C.c_long]),
    "fgoicp_multi_replay_rank": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "fgoicp_batch_create": (C.c_int, [C.POINTER(BatchPair), C.c_int, C.POINTER(BatchOpts), C.POINTER(C.c_void_p)]),
    "fgoicp_batch_run": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_int_p]),
    "fgoicp_batch_best_error": (C.c_int, [C.c_void_p, C.c_int, c_float_p]),
    "fgoicp_batch_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RunStats)]),
    "fgoicp_batch_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fgoicp_batch_refined_plane": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(PlaneResult)]),
    "fgoicp_batch_refined_robust": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RobustResult)]),
    "fgoicp_batch_refined_information": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Information)]),
    "fgoicp_batch_refine_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fgoicp_batch_test_refine": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(BatchRefine), c_int_p, c_float_p, c_float_p, C.POINTER(RobustResult), c_int_p,
                                           C.c_char_p, C.POINTER(C.c_uint64)]),
    "fgoicp_batch_destroy": (None, [C.c_void_p]),
    "fgoicp_batch_test_bounds": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, c_int_p, c_int_p, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p,
                                           c_float_p, c_float_p, C.POINTER(C.c_uint64)]),
    "fgoicp_batch_test_trim_bounds": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, c_int_p, c_int_p, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p,
                                                c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64)]),
    "fgoicp_batch_test_icp": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, c_int_p, c_float_p, c_float_p, C.POINTER(C.c_size_t), c_float_p, c_float_p,
                                        c_float_p, c_float_p, c_int_p]),
}
TRANSPORT_RCCL = 0
TRANSPORT_IN_PROCESS = 1

_lib = None


def lib_path():
    return _build.LIB_PATH


def load():
    """Returns the loaded library; raises if it is missing (build it with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built (python __graft_entry__.py build). "
            "fgoicp_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError here = the ABI header and the library disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def dev_knobs():
    """True if the loaded library is the development build (reads the FGOICP_* A/B knobs; csrc/host/knobs.hpp)."""
    return bool(load().fgoicp_dev_knobs())


def live_resources():
    """Test hook: (device allocations, pinned allocations, streams, events) the library's owning handles hold in this process."""
    out = (C.c_uint64 * 4)()
    check(load().fgoicp_test_live_resources(out), "fgoicp_test_live_resources")
    return tuple(int(v) for v in out)


def exported_symbols():
    return sorted(_SIGS)


class FgoicpError(RuntimeError):
    def __init__(self, status, where):
        lib = load()
        msg = lib.fgoicp_last_error().decode(errors="replace")
        super().__init__(f"{where} failed with status {status}: {msg}")
        self.status = status


def check(status, where):
    if status != 0:
        raise FgoicpError(status, where)
