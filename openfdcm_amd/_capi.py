"""ctypes binding of libfdcm_hip.so (include/fdcm.h).

There is no CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfdcm_hip.so")

FDCM_OK = 0
L2, L2_SQUARED, L1 = 0, 1, 2
DEFAULT_OPTIMIZE, BATCH_OPTIMIZE, INDULGENT_OPTIMIZE = 0, 1, 2
DEFAULT_PENALTY, EXPONENTIAL_PENALTY = 0, 1
GATE_WINNER, GATE_ALL = 0, 1  # FDCM_GATE_WINNER, FDCM_GATE_ALL
FOOTPRINT_BOX, FOOTPRINT_HULL = 0, 1  # FDCM_FOOTPRINT_BOX, FDCM_FOOTPRINT_HULL
SHARDED_ALWAYS_COLLECTIVE = 1
SHARDED_ALLOW_SAME_DEVICE = 2
SHARD_TEMPLATES, SHARD_FRAMES = 0, 1
# enum fdcm_poison_buffer, in its order: FDCM_FILL_EVAL = 0, .., FDCM_FILL_PIXEL_OUT (fdcm_selftest_poison_fills)
POISON_BUFFERS = ("eval", "eval_stage", "vol", "ivol", "bitmap", "coldesc", "colmask", "labels", "edge_parent", "edge_roots", "pyr", "offtab",
                  "stack", "plan", "build_stage", "scene", "pairs", "records", "flags", "work", "counter", "bins", "out", "search_stage",
                  "bins_stage", "cnt", "tail", "tail_out", "coverage", "coverage_stage", "pixel_pixels", "pixel_labels", "pixel_keys",
                  "pixel_parent", "pixel_counts", "pixel_comps", "pixel_out")

MATCH_DTYPE = np.dtype([("tmpl_idx", "<i4"), ("score", "<f4"), ("transform", "<f4", (6,))])
assert MATCH_DTYPE.itemsize == 32


class FeaturemapInfo(C.Structure):
    _fields_ = [("width", C.c_int64), ("height", C.c_int64), ("depth", C.c_int64),
                ("scene_translation", C.c_float * 2), ("distance", C.c_int32),
                ("dt3_coeff", C.c_float), ("padding", C.c_float)]


class BuildTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("seeds_ms", C.c_float), ("pass1_ms", C.c_float),
                ("pass2_ms", C.c_float), ("propagate_ms", C.c_float), ("integral_ms", C.c_float), ("span_ms", C.c_float)]


class SearchTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("kernel_ms", C.c_float), ("candidates", C.c_int64),
                ("evaluations", C.c_int64)]


class Grid(C.Structure):
    """fdcm_grid: translations (x0 + i * sx, y0 + j * sy) for 0 <= i < nx, 0 <= j < ny."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("sx", C.c_int32),
                ("sy", C.c_int32)]

    def as_tuple(self):
        return (self.x0, self.y0, self.nx, self.ny, self.sx, self.sy)

    def __repr__(self):
        return "Grid(x0={}, y0={}, nx={}, ny={}, sx={}, sy={})".format(*self.as_tuple())


class Rotations(C.Structure):
    """fdcm_rotations: n pairs (c, s) at cs, and one pivot (px, py) per template at pivots or NULL (the origin)."""
    _fields_ = [("cs", C.POINTER(C.c_float)), ("n", C.c_int32), ("pivots", C.POINTER(C.c_float))]


class PoseWindow(C.Structure):
    """fdcm_pose_window: one job of fdcm_search_exhaustive_windows: a template, a run of rotations, a translation grid."""
    _fields_ = [("tmpl", C.c_int32), ("a0", C.c_int32), ("na", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("nx", C.c_int32), ("ny", C.c_int32)]


POSE_WINDOW_DTYPE = np.dtype([(n, "<i4") for n in ("tmpl", "a0", "na", "x0", "y0", "nx", "ny")])
assert POSE_WINDOW_DTYPE.itemsize == C.sizeof(PoseWindow) == 28


class EdgeParams(C.Structure):
    """fdcm_edge_params: smoothing (0, 1, 2), the low and high thresholds and the smallest component kept."""
    _fields_ = [("smooth", C.c_int32), ("low", C.c_int32), ("high", C.c_int32), ("min_pixels", C.c_int32)]


class LineParams(C.Structure):
    """fdcm_line_params: labels per orientation bucket, the fewest pixels and the shortest extent of a kept component."""
    _fields_ = [("bucket", C.c_int32), ("min_pixels", C.c_int32), ("min_length", C.c_int32)]


class LinesTiming(C.Structure):
    """fdcm_lines_timing: device milliseconds per stage of the thread's last fdcm_lines_from_* call."""
    _fields_ = [(n, C.c_float) for n in ("edges_ms", "tiles_ms", "borders_ms", "number_ms", "sums_ms", "votes_ms", "keep_ms",
                                         "fit_ms", "total_ms")] + [("n_lines", C.c_int64)]


class CoverageParams(C.Structure):
    """fdcm_coverage_params: the radius in pixels, the circular tolerance in slices and the footprint's margin."""
    _fields_ = [("radius", C.c_int32), ("bin_tolerance", C.c_int32), ("margin", C.c_int32)]


assert C.sizeof(CoverageParams) == 12


class FitParams(C.Structure):
    """fdcm_fit_params: the steps, the fewest fit pixels a step needs, the damping's share of the diagonal, and the longest
    step per axis (pixels) and in angle (radians)."""
    _fields_ = [("iterations", C.c_int32), ("min_pixels", C.c_int32), ("damping", C.c_double), ("max_shift", C.c_double),
                ("max_angle", C.c_double)]


assert C.sizeof(FitParams) == 32


class SelectParams(C.Structure):
    """fdcm_select_params: the static test's share (explained / edges), the share of a pose's explained pixels that must be
    unclaimed at its turn, both in permille, the least number of pixels for either, and the most poses to accept."""
    _fields_ = [("min_coverage_permille", C.c_int32), ("min_new_permille", C.c_int32), ("min_pixels", C.c_int32),
                ("max_selected", C.c_int32)]


assert C.sizeof(SelectParams) == 16

MESH_VIS_ITEMS, MESH_VIS_EXACT = 0, 1  # FDCM_MESH_VIS_ITEMS, FDCM_MESH_VIS_EXACT


class MeshLineParams(C.Structure):
    """fdcm_mesh_line_params: the depth tolerance, the shortest line kept, the visibility rule and the joining tolerance
    (negative: no joining)."""
    _fields_ = [("depth_tol", C.c_float), ("min_length", C.c_float), ("visibility", C.c_int32), ("join_tolerance", C.c_float)]


assert C.sizeof(MeshLineParams) == 16


class MeshCamera(C.Structure):
    """fdcm_mesh_camera: the focal length in pixels and the near distance in mesh units."""
    _fields_ = [("focal", C.c_float), ("near", C.c_float)]


assert C.sizeof(MeshCamera) == 8

# every symbol include/fdcm.h declares: (name, restype, argtypes)
_fp, _i64p, _vp = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.c_void_p
SYMBOLS = [
    ("fdcm_last_error", C.c_char_p, []),
    ("fdcm_version", C.c_char_p, []),
    ("fdcm_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("fdcm_set_device", C.c_int, [C.c_int]),
    ("fdcm_get_device", C.c_int, [C.POINTER(C.c_int)]),
    ("fdcm_featuremap_build", C.c_int, [_fp, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_int, C.POINTER(_vp)]),
    ("fdcm_featuremap_rebuild", C.c_int, [_vp, _fp, C.c_int64]),
    ("fdcm_featuremap_free", C.c_int, [_vp]),
    ("fdcm_featuremap_get_info", C.c_int, [_vp, C.POINTER(FeaturemapInfo)]),
    ("fdcm_featuremap_keys", C.c_int, [_vp, _fp]),
    ("fdcm_featuremap_slice", C.c_int, [_vp, C.c_int64, _fp]),
    ("fdcm_featuremap_device_volume", C.c_int, [_vp, C.POINTER(_vp)]),
    ("fdcm_featuremap_device_volume_stride", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("fdcm_featuremap_last_timing", C.c_int, [_vp, C.POINTER(BuildTiming)]),
    ("fdcm_featuremap_stage_timing", C.c_int, [_vp, C.c_int]),
    ("fdcm_featuremap_from_slices", C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int64, _fp, C.POINTER(_vp)]),
    ("fdcm_featuremap_build_staged", C.c_int,
     [_fp, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("fdcm_edge_labels", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, _vp]),
    ("fdcm_featuremap_build_image", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                              C.c_float, C.c_int, C.POINTER(_vp)]),
    ("fdcm_featuremap_rebuild_image", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64]),
    ("fdcm_featuremap_build_labels", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_int,
                                               C.POINTER(_vp)]),
    ("fdcm_featuremap_rebuild_labels", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, C.c_int64]),
    ("fdcm_featuremap_build_image_staged", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64,
                                                     C.c_int64, C.c_float, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("fdcm_edge_labels_ex", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(EdgeParams), _vp]),
    ("fdcm_featuremap_build_image_ex", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(EdgeParams), C.c_int64,
                                                 C.c_int64, C.c_float, C.c_int, C.POINTER(_vp)]),
    ("fdcm_featuremap_rebuild_image_ex", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(EdgeParams),
                                                   C.c_int64]),
    ("fdcm_image_pyramid_size", C.c_int, [C.c_int64, C.c_int64, C.c_int32, _i64p, _i64p]),
    ("fdcm_image_pyramid_level", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int32, _vp, C.c_int]),
    ("fdcm_featuremap_build_image_level", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int32, C.POINTER(EdgeParams),
                                                    C.c_int64, C.c_int64, C.c_float, C.c_int, C.POINTER(_vp)]),
    ("fdcm_featuremap_rebuild_image_level", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int32,
                                                      C.POINTER(EdgeParams), C.c_int64]),
    ("fdcm_featuremap_minmax_translation", C.c_int, [_vp, _fp, C.c_int64, _fp, _fp]),
    ("fdcm_featuremap_minmax_translation_batch", C.c_int, [_vp, _fp, _i64p, C.c_int64, _fp, _fp]),
    ("fdcm_featuremap_evaluate", C.c_int, [_vp, _fp, _i64p, C.c_int64, _fp, _i64p, _fp]),
    ("fdcm_templates_create", C.c_int, [_fp, _i64p, C.c_int64, C.POINTER(_vp)]),
    ("fdcm_templates_free", C.c_int, [_vp]),
    ("fdcm_templates_count", C.c_int, [_vp, _i64p, _i64p]),
    ("fdcm_templates_lengths", C.c_int, [_vp, _fp]),
    ("fdcm_search", C.c_int, [_vp, _vp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int32,
                              C.POINTER(_vp), _i64p]),
    ("fdcm_search_capacity", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _i64p]),
    ("fdcm_search_device", C.c_int, [_vp, _vp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int32,
                                     _vp, _i64p]),
    ("fdcm_search_last_timing", C.c_int, [_vp, C.POINTER(SearchTiming)]),
    ("fdcm_matches_free", None, [_vp]),
    ("fdcm_blocks_to_host", C.c_int, [_vp, C.c_int32, C.c_int64, _vp, C.POINTER(_vp), C.POINTER(C.c_int64)]),
    ("fdcm_topk", C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int, C.c_float, C.c_int64, C.POINTER(_vp), _i64p]),
    ("fdcm_pipeline_create", C.c_int, [C.c_int64, C.c_float, C.c_float, C.c_int, _vp, C.c_int64, C.c_int64, C.c_int,
                                       C.c_int64, C.c_int32, C.c_int, C.POINTER(_vp)]),
    ("fdcm_pipeline_submit", C.c_int, [_vp, _fp, C.c_int64, _vp, _i64p]),
    ("fdcm_pipeline_wait", C.c_int, [_vp, C.c_int64, C.POINTER(_vp), _i64p, C.POINTER(BuildTiming),
                                     C.POINTER(SearchTiming)]),
    ("fdcm_pipeline_slots", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("fdcm_pipeline_free", C.c_int, [_vp]),
    ("fdcm_sharded_create", C.c_int, [C.POINTER(C.c_int), C.c_int, _fp, _i64p, C.c_int64, C.c_int64, C.c_float, C.c_float,
                                      C.c_int, C.c_int, C.POINTER(_vp)]),
    ("fdcm_sharded_search", C.c_int, [_vp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(_vp), _i64p]),
    ("fdcm_sharded_search_topk", C.c_int, [_vp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_float,
                                           C.c_int64, C.POINTER(_vp), _i64p]),
    ("fdcm_sharded_set_frames_in_flight", C.c_int, [_vp, C.c_int]),
    ("fdcm_sharded_set_mode", C.c_int, [_vp, C.c_int]),
    ("fdcm_sharded_submit", C.c_int, [_vp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, _i64p]),
    ("fdcm_sharded_submit_topk", C.c_int, [_vp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_float,
                                           C.c_int64, _i64p]),
    ("fdcm_sharded_wait", C.c_int, [_vp, C.c_int64, C.POINTER(_vp), _i64p]),
    ("fdcm_sharded_info", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), _i64p, _i64p, _i64p]),
    ("fdcm_sharded_last_timing", C.c_int, [_vp, C.c_int, C.POINTER(BuildTiming), C.POINTER(SearchTiming)]),
    ("fdcm_sharded_free", C.c_int, [_vp]),
    ("fdcm_filter_in_range", C.c_int, [_fp, C.c_int64, _fp, C.c_float, C.c_float, _i64p, _i64p]),
    ("fdcm_penalize", C.c_int, [C.c_int, C.c_float, _vp, C.c_int64, _fp, C.c_int64]),
    ("fdcm_sort_matches", C.c_int, [_vp, C.c_int64]),
    ("fdcm_partial_sort_matches", C.c_int, [_vp, C.c_int64, C.c_int64]),
    ("fdcm_exhaustive_window", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.POINTER(Grid)]),
    ("fdcm_search_exhaustive", C.c_int, [_vp, _vp, C.POINTER(Grid), C.c_int32, C.c_int32, C.POINTER(_vp), _i64p]),
    ("fdcm_search_exhaustive_peaks", C.c_int, [_vp, _vp, C.POINTER(Grid), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(_vp), _i64p]),
    ("fdcm_score_map", C.c_int, [_vp, _vp, C.POINTER(Grid), _fp]),
    ("fdcm_exhaustive_rotations_window", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.c_int32, C.c_int32, C.POINTER(Grid)]),
    ("fdcm_search_exhaustive_rotations", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp), _i64p]),
    ("fdcm_score_map_rotations", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), _fp]),
    ("fdcm_search_exhaustive_windows", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(PoseWindow), C.c_int64, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp), _i64p, _i64p]),
    ("fdcm_score_map_device", C.c_int, [_vp, _vp, C.POINTER(Grid), _vp]),
    ("fdcm_best_map", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_int, C.c_float, _fp, C.POINTER(C.c_int32)]),
    ("fdcm_search_exhaustive_detect", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int, C.c_float, C.c_int32, C.POINTER(_vp), _i64p]),
    ("fdcm_search_exhaustive_detect_nms", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int, C.c_float, C.c_int32, C.POINTER(_vp), C.POINTER(C.c_int32), _i64p]),
    ("fdcm_search_exhaustive_detect_all", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_float, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_int, C.c_float, C.c_int32, C.POINTER(_vp), _i64p,
                                                   C.POINTER(C.c_int32)]),
    ("fdcm_search_exhaustive_detect_all_matched", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_float, C.c_int32,
                                                           C.c_int32, C.c_int32, C.c_int, C.c_float, C.c_float, C.c_int32,
                                                           C.POINTER(_vp), _i64p, C.POINTER(C.c_int32), _fp]),
    ("fdcm_search_exhaustive_detect_windows", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(PoseWindow), C.c_int64, C.c_int32,
                                                       C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int,
                                                       C.c_float, C.c_float, C.c_int32, C.POINTER(_vp), _i64p, C.POINTER(C.c_int32),
                                                       _fp, C.POINTER(C.c_int32)]),
    ("fdcm_best_map_gated", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_int, C.c_float, C.c_float, _fp,
                                     C.POINTER(C.c_int32), _fp]),
    ("fdcm_search_exhaustive_detect_all_gated", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_float, C.c_int32,
                                                         C.c_int32, C.c_int32, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int32,
                                                         C.POINTER(_vp), _i64p, C.POINTER(C.c_int32), _fp]),
    ("fdcm_search_exhaustive_detect_windows_gated", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(PoseWindow), C.c_int64,
                                                             C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                                             C.c_int32, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int32,
                                                             C.POINTER(_vp), _i64p, C.POINTER(C.c_int32), _fp, C.POINTER(C.c_int32)]),
    ("fdcm_best_map_objects", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.c_int, C.c_float, C.POINTER(C.c_int32),
                                       C.c_int32, _fp, _fp, C.POINTER(C.c_int32), _fp]),
    ("fdcm_search_exhaustive_detect_objects", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(Grid), C.POINTER(C.c_int32), C.c_int32,
                                                       _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_float, C.c_int,
                                                       C.c_int32, C.POINTER(_vp), _i64p, C.POINTER(C.c_int32), _fp]),
    ("fdcm_search_exhaustive_detect_windows_objects", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(PoseWindow), C.c_int64,
                                                               C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _fp, _fp,
                                                               C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_float, C.c_int,
                                                               C.c_int32, C.POINTER(_vp), _i64p, C.POINTER(C.c_int32), _fp,
                                                               C.POINTER(C.c_int32)]),
    ("fdcm_matched_fractions", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(C.c_int32), C.c_int64, _fp]),
    ("fdcm_templates_matched_totals", C.c_int, [_vp, _fp]),
    ("fdcm_detect_score_bounds", C.c_int, [_vp, C.c_int, C.c_float, C.c_float, _fp]),
    ("fdcm_score_bound", C.c_int, [C.c_float, C.c_float, _fp]),
    ("fdcm_templates_footprints", C.c_int, [_vp, C.POINTER(Rotations), C.c_int32, C.POINTER(C.c_int32)]),
    ("fdcm_lines_footprints", C.c_int, [_fp, _i64p, C.c_int64, C.POINTER(Rotations), C.c_int32, C.POINTER(C.c_int32)]),
    ("fdcm_templates_create_capped", C.c_int, [_fp, _i64p, C.c_int64, _fp, C.POINTER(_vp)]),
    ("fdcm_templates_create_shaped", C.c_int, [_fp, _i64p, C.c_int64, _fp, C.c_int32, C.POINTER(_vp)]),
    ("fdcm_templates_footprint_kind", C.c_int, [_vp, C.POINTER(C.c_int32)]),
    ("fdcm_templates_footprint_spans", C.c_int, [_vp, C.POINTER(Rotations), C.c_int32, _i64p, _i64p, C.POINTER(C.c_int32)]),
    ("fdcm_lines_footprint_spans", C.c_int, [_fp, _i64p, C.c_int64, C.POINTER(Rotations), C.c_int32, _i64p, _i64p,
                                             C.POINTER(C.c_int32)]),
    ("fdcm_templates_line_caps", C.c_int, [_vp, _fp]),
    ("fdcm_templates_line_lengths", C.c_int, [_vp, _fp]),
    ("fdcm_line_costs", C.c_int, [_vp, _vp, C.POINTER(Rotations), C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.POINTER(C.c_float)),
                                  _i64p]),
    ("fdcm_scene_coverage", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, C.POINTER(Rotations), C.POINTER(C.c_int32), C.c_int64,
                                      C.POINTER(CoverageParams), C.POINTER(C.c_int32), _vp]),
    ("fdcm_scene_select", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, C.POINTER(Rotations), C.POINTER(C.c_int32), C.c_int64,
                                    C.POINTER(CoverageParams), C.POINTER(SelectParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i64p,
                                    _vp]),
    ("fdcm_matches_footprints", C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("fdcm_matches_verify", C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int32, _fp, _fp, _fp]),
    ("fdcm_matches_detect", C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int,
                                      C.c_float, C.c_float, C.c_int, C.POINTER(_vp), _i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      _fp]),
    ("fdcm_matches_detect_objects", C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _fp, _fp,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_float, C.c_int, C.POINTER(_vp),
                                              _i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp]),
    ("fdcm_matches_footprint_spans", C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _i64p, _i64p, C.POINTER(C.c_int32)]),
    ("fdcm_matches_shapes", C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int32, C.c_int32, _i64p, _i64p, C.POINTER(C.c_int32)]),
    ("fdcm_matches_coverage", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, _vp, C.c_int64, C.c_int, C.c_int32,
                                        C.POINTER(CoverageParams), C.POINTER(C.c_int32), _vp]),
    ("fdcm_matches_select", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, _vp, C.c_int64, C.c_int, C.c_int32,
                                      C.POINTER(CoverageParams), C.POINTER(SelectParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i64p,
                                      _vp]),
    ("fdcm_matches_refine", C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int32, C.POINTER(Rotations), C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, _vp, C.c_int, C.POINTER(C.c_int32)]),
    ("fdcm_matches_fit", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, _vp, C.c_int64, C.c_int, C.c_int32,
                                   C.POINTER(CoverageParams), C.POINTER(FitParams), _vp, C.c_int, C.POINTER(C.c_int32), _fp]),
    ("fdcm_lines_read", C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int64)]),
    ("fdcm_lines_write", C.c_int, [C.c_char_p, _fp, C.c_int64]),
    ("fdcm_lines_free", None, [C.POINTER(C.c_float)]),
    ("fdcm_lines_from_labels", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(LineParams),
                                         C.POINTER(C.POINTER(C.c_float)), _i64p]),
    ("fdcm_lines_from_image", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(EdgeParams),
                                        C.POINTER(LineParams), C.POINTER(C.POINTER(C.c_float)), _i64p]),
    ("fdcm_lines_last_timing", C.c_int, [C.POINTER(LinesTiming)]),
    ("fdcm_mesh_create", C.c_int, [_fp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_double, C.POINTER(_vp)]),
    ("fdcm_mesh_free", C.c_int, [_vp]),
    ("fdcm_mesh_info", C.c_int, [_vp, _i64p, _i64p, _i64p]),
    ("fdcm_mesh_edges", C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]),
    ("fdcm_mesh_view_lines", C.c_int, [_vp, _fp, C.c_int64, C.c_float, C.c_float, C.c_float, C.POINTER(C.POINTER(C.c_float)), _i64p]),
    ("fdcm_mesh_view_lines_ex", C.c_int, [_vp, _fp, C.c_int64, C.c_float, C.POINTER(MeshLineParams), C.POINTER(C.POINTER(C.c_float)), _i64p]),
    ("fdcm_mesh_view_items", C.c_int, [_vp, _fp, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_int64]),
    ("fdcm_mesh_view_lines_cam", C.c_int, [_vp, _fp, _fp, C.c_int64, C.POINTER(MeshCamera), C.POINTER(MeshLineParams),
                                           C.POINTER(C.POINTER(C.c_float)), _i64p]),
    ("fdcm_mesh_view_items_cam", C.c_int, [_vp, _fp, _fp, C.POINTER(MeshCamera), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_int64]),
    ("fdcm_selftest_atanf", C.c_int64, [C.c_uint32, C.c_uint32, C.c_uint64]),
    ("fdcm_orientation_bins_mode", C.c_int, []),
    ("fdcm_selftest_sweep_ranges", C.c_int, [C.c_int]),
    ("fdcm_selftest_sweep_order_counts", C.c_int, [_i64p, _i64p]),
    ("fdcm_selftest_sweep_steals", C.c_int, [_vp, _i64p]),
    ("fdcm_selftest_poison_fills", C.c_int, [C.POINTER(C.c_int32), C.c_int64, _i64p]),
]

_lib = None


class FdcmError(RuntimeError):
    pass


def loaded():
    """True once libfdcm_hip.so (and with it /opt/rocm's HIP runtime) is in the process."""
    return _lib is not None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FdcmError(
                f"{LIB_PATH} is missing: build it with `make -C openfdcm_amd/csrc` (or __graft_entry__.build()); "
                "openfdcm_amd has no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc):
    if rc != FDCM_OK:
        raise FdcmError(f"libfdcm_hip: {lib().fdcm_last_error().decode()} (code {rc})")


def fptr(a):
    return a.ctypes.data_as(_fp)


def as_records(lines):
    """(4, N) array-like (the reference's LineArray) -> (N, 4) contiguous float32 records."""
    a = np.asarray(lines, dtype=np.float32)
    if a.ndim == 1 and a.size % 4 == 0:
        a = a.reshape(4, -1)
    if a.ndim != 2 or a.shape[0] != 4:
        raise ValueError(f"expected a (4, N) line array, got shape {a.shape}")
    return np.ascontiguousarray(a.T)


def pack_templates(templates):
    """list of (4, N_i) LineArrays -> ((sum N_i, 4) float32 records, int64 offsets of length len + 1)."""
    n = len(templates)
    offsets = np.zeros(n + 1, dtype=np.int64)
    if n and all(isinstance(t, np.ndarray) and t.ndim == 2 and t.shape[0] == 4 for t in templates):
        # the usual case in one concatenate instead of a transpose + copy per template
        np.cumsum([t.shape[1] for t in templates], out=offsets[1:])
        if offsets[-1] == 0:
            return np.zeros((0, 4), dtype=np.float32), offsets
        return np.ascontiguousarray(np.concatenate(templates, axis=1).T, dtype=np.float32), offsets
    recs = [as_records(t) for t in templates]
    for i, r in enumerate(recs):
        offsets[i + 1] = offsets[i] + r.shape[0]
    if recs and offsets[-1] > 0:
        flat = np.ascontiguousarray(np.concatenate(recs, axis=0), dtype=np.float32)
    else:
        flat = np.zeros((0, 4), dtype=np.float32)
    return flat, offsets
