"""ctypes binding of libroam_hip.so (include/roam_abi.h).  No torch, no CPU fallback: if
the HIP library or a gfx950 device is missing every compute call raises RoamError."""
import ctypes as C
import numbers
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ROAM_LIB") or os.path.join(_HERE, "csrc", "libroam_hip.so")     # ROAM_LIB: an A/B build (profiles/build_variant.py)

ROAM_OK, ROAM_E_ARG, ROAM_E_HIP, ROAM_E_CAPACITY, ROAM_E_NODEVICE, ROAM_E_STATE = 0, -1, -2, -3, -4, -5
WARP_POLAR_LOG, WARP_POLAR_INVERSE = 1, 2      # roam_abi.h ROAM_WARP_POLAR_*
WARP_AFFINE_INVERSE_MAP = 1     # roam_abi.h ROAM_WARP_AFFINE_INVERSE_MAP
WARP_AFFINE_MAX_SIDE = 16384    # largest image side of roam_warp_affine_f32
WARP_AFFINE_MAX_COORD = 2.0 ** 20   # source coordinates (px) the fixed-point sums of roam_warp_affine_f32 hold without overflow
TIME_FFT_FIVE, TIME_DFT_FIVE, TIME_FFT_ROWS, TIME_FFT_TRANSPOSE, TIME_FFT_COLS = range(5)      # roam_abi.h ROAM_TIME_*
PHASE_CORRELATE_MAX = 4096      # largest image side of roam_phase_correlate_f32
FMT_MIN_R, FMT_MAX_R = 4, 1303  # roam_abi.h ROAM_FMT_MIN_R / ROAM_FMT_MAX_R: columns after the resize of the batched rotation prior
FMT_MAX_ROWS = 16384            # ... and its largest number of polar rows
FMT_MAX_COLS = 16384            # widest polar image the Cartesian half of the registration reads (roam_fmt_register_batch_f32)
MAX_FEATURES = 1024
STEP_NEW_SEQUENCE = 0x40000000      # roam_abi.h ROAM_STEP_NEW_SEQUENCE: OR into a lane's scan index


class RoamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libroam_hip error {code}: {msg}")
        self.code = code


class EngineCfg(C.Structure):
    _fields_ = [("lanes", C.c_int32), ("rows", C.c_int32), ("stride", C.c_int32), ("payload_off", C.c_int32),
                ("clip", C.c_int32), ("pool_scans", C.c_int32), ("peaks_cap", C.c_int32),
                ("reject_outliers", C.c_int32), ("motion_distortion", C.c_int32),
                ("clique_node_limit", C.c_int64), ("sigma5", C.c_double * 5), ("retrack_on_device", C.c_int32),
                ("retrack_slots", C.c_int32), ("keyframe_trans_m", C.c_double), ("keyframe_rot_rad", C.c_double)]


class LaneResult(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("velocity", C.c_double * 3), ("kabsch_R", C.c_double * 4),
                ("kabsch_h", C.c_double * 2), ("n_tracked", C.c_int32), ("n_good", C.c_int32),
                ("n_inliers", C.c_int32), ("n_peaks", C.c_int32), ("lm_nfev", C.c_int32),
                ("lm_info", C.c_int32), ("flags", C.c_int32), ("n_after_retrack", C.c_int32)]


class AutoPriorCfg(C.Structure):
    """roam_abi.h roam_auto_prior_cfg"""
    _fields_ = [("clip_px", C.c_int32), ("downsample", C.c_int32), ("cart_downsample", C.c_int32),
                ("min_rot_response", C.c_double), ("min_trans_response", C.c_double)]


class PoseGraphOpts(C.Structure):
    """roam_abi.h roam_pose_graph_opts"""
    _fields_ = [("max_iterations", C.c_int32), ("max_trials", C.c_int32), ("lambda_init", C.c_double)]


# roam_abi.h roam_pose_graph_stats, one row per graph
POSE_GRAPH_STATS = np.dtype([("iterations", np.int32), ("trials", np.int32), ("rejected", np.int32), ("stop", np.int32),
                             ("chi2_initial", np.float64), ("chi2_final", np.float64), ("lambda_final", np.float64)])
POSE_GRAPH_MAX_GRAPHS = 65535           # limits of roam_pose_graph_optimize
POSE_GRAPH_MAX_VERTICES = 32768
POSE_GRAPH_MAX_ITERATIONS = 1000
POSE_GRAPH_MAX_TRIALS = 1000
POSE_GRAPH_CHUNK_BYTES = 2000 << 20     # device scratch of one launch

class IcpOpts(C.Structure):
    """roam_abi.h roam_icp_opts"""
    _fields_ = [("gate_start", C.c_double), ("gate_end", C.c_double), ("gate_decay", C.c_double), ("max_iterations", C.c_int32),
                ("eps_trans", C.c_double), ("eps_rot", C.c_double), ("min_pairs", C.c_int32)]


# roam_abi.h roam_icp_stats, one row per pair
ICP_STATS = np.dtype([("status", np.int32), ("iterations", np.int32), ("n_pairs_last", np.int32), ("n_inliers", np.int32),
                      ("rms", np.float64)])
IcpStats = ICP_STATS
ICP_OK, ICP_MAX_ITERATIONS, ICP_FEW_PAIRS = 0, 1, 2     # roam_abi.h ROAM_ICP_*: the status of a pair
ICP_MAX_PAIRS, ICP_MAX_POINTS = 65535, 8192             # limits of roam_icp2d_batch
ICP_MAX_COORD = 1e6
ICP_ITERATION_LIMIT = 1000
ICP_DEFAULTS = dict(gate_start=3.0, gate_end=0.5, gate_decay=0.8, max_iterations=40, eps_trans=1e-4, eps_rot=1e-5, min_pairs=3)

SCAN_CONTEXT_MAX_SECTORS, SCAN_CONTEXT_MAX_RINGS = 256, 128     # roam_abi.h ROAM_SCAN_CONTEXT_MAX_*
SCAN_CONTEXT_MAX_ROWS, SCAN_CONTEXT_MAX_CLIP = 65536, 4096
LOOP_MAX_K = 32                         # roam_abi.h ROAM_LOOP_MAX_K
LOOP_MAX_OFFSETS = 48                   # roam_abi.h ROAM_LOOP_MAX_OFFSETS
LOOP_DB_BYTES = 2000 << 20              # a database, and the device scratch of one launch
MAP_MAX_CELLS = 1 << 26                 # roam_abi.h ROAM_MAP_MAX_CELLS: the cells of a global map's grid


PRIOR_RECORD = np.dtype([("out6", np.float64, (6,)), ("affine", np.float32, (2, 3)), ("source", np.uint8)])     # Engine.step_prior's rows


class KeyframeHdr(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("velocity", C.c_double * 3), ("n_features", C.c_int32), ("n_peaks", C.c_int32),
                ("scan", C.c_int32), ("lane", C.c_int32)]


COMM_ID_BYTES = 128
_P = C.POINTER
_vp = C.c_void_p
_SIGS = {
    "roam_create": (C.c_int32, [C.c_int32, _P(_vp)]),
    "roam_destroy": (C.c_int32, [_vp]),
    "roam_last_error": (C.c_char_p, [_vp]),
    "roam_version": (C.c_char_p, []),
    "roam_device_info": (C.c_int32, [_vp, C.c_char_p, C.c_int32, _P(C.c_int32), _P(C.c_int64), C.c_char_p, C.c_int32]),
    "roam_synchronize": (C.c_int32, [_vp]),
    "roam_host_alloc": (C.c_int32, [_vp, C.c_int64, _P(_vp)]),
    "roam_host_free": (C.c_int32, [_vp, _vp]),
    "roam_png_decode_gray8": (C.c_int32, [_vp, C.c_int64, _vp, C.c_int64, C.c_int64, _P(C.c_int32), _P(C.c_int32)]),
    "roam_png_decode_file": (C.c_int32, [C.c_char_p, _vp, C.c_int64, C.c_int64, _P(C.c_int32), _P(C.c_int32)]),
    "roam_png_pool_create": (C.c_int32, [C.c_int32, _P(_vp)]),
    "roam_png_pool_submit": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_int64, C.c_int64, C.c_int64]),
    "roam_png_pool_wait": (C.c_int32, [_vp, C.c_int64, _P(C.c_int32), _P(C.c_int32)]),
    "roam_png_pool_destroy": (C.c_int32, [_vp]),
    "roam_peaks_polar_f32": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int64, _P(C.c_int64)]),
    "roam_peaks_record_u8": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_int64, _P(C.c_int64)]),
    "roam_peaks_polar_f32_cond": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, _vp, C.c_int64,
                                              _P(C.c_int64)]),
    "roam_peaks_record_u8_cond": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                              _vp, C.c_int64, _P(C.c_int64)]),
    "roam_polar_to_cart_f32": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    "roam_polar_to_cart_record_u8": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "roam_warp_polar_f32": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _vp, C.c_int32, C.c_int32,
                                        C.c_float, C.c_float, C.c_double, C.c_int32]),
    "roam_warp_affine_f32": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _vp, C.c_int32, _vp, C.c_int32,
                                         C.c_int32, C.c_int32]),
    "roam_time_warp_affine": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _P(C.c_float)]),
    "roam_klt_track_u8": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "roam_klt_track_f32": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "roam_klt_track_u8_flow": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "roam_klt_track_f32_flow": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "roam_pyr_down_u8": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    "roam_reject_outliers": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_double, C.c_int64, _vp, _P(C.c_int32), _P(C.c_int32), _vp]),
    "roam_time_reject_outliers": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_double, C.c_int64, C.c_int32, _P(C.c_float), _P(C.c_float),
                                               _P(C.c_int32), _P(C.c_int32)]),
    "roam_kabsch2d": (C.c_int32, [_vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "roam_mds_solve": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_double, _vp, _P(C.c_int32), _P(C.c_int32), _vp, _vp]),
    "roam_mds_undistort": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_double, _vp, _vp]),
    "roam_ssc": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, _vp, _P(C.c_int32)]),
    "roam_doh_maxima": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_double, _vp, _vp, C.c_int32, _P(C.c_int32)]),
    "roam_log_maxima": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_double, _vp, _vp, C.c_int32,
                                    _P(C.c_int32), _vp]),
    "roam_pose_graph_plan": (C.c_int32, [C.c_int32, _vp, _vp, _vp, _vp, _vp, _P(C.c_int64)]),
    "roam_pose_graph_optimize": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(PoseGraphOpts), _vp]),
    "roam_scan_context_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "roam_scan_context_f32": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_double, _vp]),
    "roam_loop_db_create": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int32, _P(_vp)]),
    "roam_loop_db_destroy": (C.c_int32, [_vp, _vp]),
    "roam_loop_db_count": (C.c_int32, [_vp, _P(C.c_int32)]),
    "roam_loop_db_add_f32": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double,
                                         _P(C.c_int32)]),
    "roam_loop_db_add_desc": (C.c_int32, [_vp, _vp, _vp, C.c_int32, _P(C.c_int32)]),
    "roam_loop_db_get": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    "roam_engine_loop_db_add": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, _P(C.c_int32)]),
    "roam_loop_db_query": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "roam_engine_time_loop_describe": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _P(C.c_float)]),
    "roam_time_loop_db_query": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, C.c_int32, _P(C.c_float), _P(C.c_float)]),
    "roam_polar_cloud_table": (C.c_int32, [C.c_int32, _vp, _vp]),
    "roam_loop_db_keep_clouds": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    "roam_loop_db_set_cloud": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32]),
    "roam_loop_db_get_cloud": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "roam_loop_db_cloud_counts": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    "roam_loop_db_verify": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _P(IcpOpts), _vp, _vp]),
    "roam_loop_db_query_verify": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, _P(IcpOpts), _vp, _vp, _vp, _vp, _vp]),
    "roam_engine_time_loop_cloud": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, _P(C.c_float), _P(C.c_float)]),
    "roam_time_loop_db_verify": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _P(IcpOpts), C.c_int32, _P(C.c_float)]),
    "roam_scan_context_offset_table": (C.c_int32, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "roam_loop_db_keep_offsets": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_double]),
    "roam_loop_db_set_variants": (C.c_int32, [_vp, _vp, C.c_int32, _vp]),
    "roam_loop_db_get_variants": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp]),
    "roam_scan_context_offsets_f32": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_double, C.c_int32, _vp, C.c_double, _vp]),
    "roam_loop_db_query_offsets": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "roam_loop_db_query_verify_offsets": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, _P(IcpOpts), _vp, _vp, _vp, _vp, _vp,
                                                      _vp]),
    "roam_engine_time_loop_offsets": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _P(C.c_float)]),
    "roam_time_loop_db_query_offsets": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, C.c_int32, _P(C.c_float), _P(C.c_float),
                                                    _P(C.c_float)]),
    "roam_map_pose_table": (C.c_int32, [C.c_int32, _vp, _vp]),
    "roam_map_plan": (C.c_int32, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P(C.c_double), _P(C.c_double), _P(C.c_int32),
                                  _P(C.c_int32)]),
    "roam_loop_db_map_bounds": (C.c_int32, [_vp, _vp, _vp, _vp, _vp, _P(C.c_int64)]),
    "roam_loop_db_map_render": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp,
                                            _vp, _vp, _vp, _vp, C.c_int32, _P(C.c_int32), _P(C.c_int64)]),
    "roam_time_loop_db_map": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, _vp]),
    "roam_icp2d_batch": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _P(IcpOpts), _vp, _vp]),
    "roam_time_icp2d_batch": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _P(IcpOpts), C.c_int32, _P(C.c_float)]),
    "roam_engine_create": (C.c_int32, [_vp, _P(EngineCfg)]),
    "roam_engine_destroy": (C.c_int32, [_vp]),
    "roam_engine_upload_scan": (C.c_int32, [_vp, C.c_int32, _vp]),
    "roam_engine_upload_scans_async": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, C.c_int64]),
    "roam_engine_fence": (C.c_int32, [_vp]),
    "roam_engine_copy_scan": (C.c_int32, [_vp, C.c_int32, C.c_int32]),
    "roam_engine_init_lane": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp]),
    "roam_engine_step": (C.c_int32, [_vp, _vp]),
    "roam_engine_results": (C.c_int32, [_vp, _P(LaneResult), C.c_int32]),
    "roam_engine_step_results": (C.c_int32, [_vp, C.c_int64, _P(LaneResult), C.c_int32]),
    "roam_engine_steps_enqueued": (C.c_int32, [_vp, _P(C.c_int64)]),
    "roam_engine_set_retrack": (C.c_int32, [_vp, C.c_int32]),
    "roam_engine_set_motion_prior": (C.c_int32, [_vp, _vp, _vp]),
    "roam_engine_set_auto_prior": (C.c_int32, [_vp, _P(AutoPriorCfg)]),
    "roam_engine_step_prior": (C.c_int32, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int32]),
    "roam_engine_init_lane_detect": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp]),
    "roam_engine_init_lanes_detect": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    "roam_engine_lane_features": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int32, _P(C.c_int32)]),
    "roam_engine_lane_peaks": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _P(C.c_int64)]),
    "roam_engine_doh_maxima": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int32, C.c_double, _vp, _vp, C.c_int32, _P(C.c_int32)]),
    "roam_engine_fmt_rotation": (C.c_int32, [_vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, _vp]),
    "roam_engine_fmt_register": (C.c_int32, [_vp, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "roam_engine_lane_image": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, C.c_int64]),
    "roam_engine_set_features": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int32]),
    "roam_engine_kernel_avg": (C.c_int32, [_vp, C.c_char_p, C.c_int32, _P(C.c_float), _P(C.c_int32)]),
    "roam_engine_kernel_chunk_ms": (C.c_int32, [_vp, C.c_char_p, C.c_int32, _P(C.c_float), C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "roam_engine_detect_chunk": (C.c_int32, [_vp, _P(C.c_int32)]),
    "roam_engine_map_reserve": (C.c_int32, [_vp, C.c_int32]),
    "roam_engine_map_count": (C.c_int32, [_vp, C.c_int32, _P(C.c_int32)]),
    "roam_engine_map_get": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "roam_engine_stage_times": (C.c_int32, [_vp, _vp, _P(C.c_char_p), C.c_int32, _P(C.c_int32)]),
    "roam_engine_set_stage_events": (C.c_int32, [_vp, C.c_int32]),
    "roam_engine_time_kernel": (C.c_int32, [_vp, C.c_char_p, C.c_int32, _P(C.c_float), _P(C.c_double)]),
    "roam_engine_debug_detect": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp]),
    "roam_engine_debug_blobs": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "roam_fmt_rotation": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "roam_phase_correlate_f32": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _vp, _vp]),
    "roam_fmt_rotation_batch_f32": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                                _vp, _vp]),
    "roam_fmt_register_batch_f32": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                                C.c_int32, _vp, _vp]),
    "roam_debug_fft2_f64": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "roam_time_fft2": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_float)]),
    "roam_debug_ssc_batch": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                         _vp, _vp]),
    "roam_debug_mds_solve_batch": (C.c_int32, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_double, C.c_int32,
                                               C.c_int32, _vp, _vp, _vp, _vp]),
    "roam_debug_lm_lmpar": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int32, _vp, _vp, _vp]),
    "roam_prune_blobs": (C.c_int32, [_vp, C.c_int32, C.c_double, _vp]),
    "roam_debug_prune_pairs": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int32, _vp]),
    "roam_argsort_np122": (C.c_int32, [_vp, C.c_int32, _vp]),
    "roam_comm_available": (C.c_int32, []),
    "roam_comm_unique_id": (C.c_int32, [_vp]),
    "roam_comm_init": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32]),
    "roam_comm_destroy": (C.c_int32, [_vp]),
    "roam_comm_info": (C.c_int32, [_vp, _P(C.c_int32), _P(C.c_int32)]),
    "roam_comm_allreduce_f64": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32]),
    "roam_comm_barrier": (C.c_int32, [_vp]),
    "roam_bcast_keyframe": (C.c_int32, [_vp, C.c_int32, C.c_int32, _P(KeyframeHdr), _vp, C.c_int32, _vp, C.c_int64]),
    "roam_keyframe_exchange": (C.c_int32, [_vp, C.c_int32]),
    "roam_remote_map_reserve": (C.c_int32, [_vp, C.c_int32]),
    "roam_remote_map_count": (C.c_int32, [_vp, _P(C.c_int64), _P(C.c_int32)]),
    "roam_debug_keyframe_append": (C.c_int32, [_vp, _vp, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "roam_remote_map_get": (C.c_int32, [_vp, C.c_int32, _P(KeyframeHdr), _P(C.c_int32), _vp, C.c_int32, _vp, C.c_int64]),
}
ABI_SYMBOLS = tuple(_SIGS)
# entry points for the tests only: exported by the library, not declared in include/roam_abi.h
_INTERNAL_SIGS = {
    "roam_pyr_down2_u8": (C.c_int32, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                      _P(C.c_int32)]),
}


def peak_conditions(distance=None, prominence=None):
    """find_peaks' `distance` / `prominence` arguments as they are checked and unpacked there -> (distance, prom_min, prom_max) of
    roam_peaks_*_cond: 0 = no distance condition, NaN = no bound.  distance < 1: ValueError, as find_peaks raises it.  prominence is
    pmin or a 2-sequence (pmin, pmax), either entry None; per-sample (array) bounds are not supported: NotImplementedError."""
    if distance is not None and distance < 1:
        raise ValueError('`distance` must be greater or equal to 1')
    pmin = pmax = None
    if prominence is not None:
        try:
            pmin, pmax = prominence                  # scipy.signal._peak_finding._unpack_condition_args
        except (TypeError, ValueError):
            pmin, pmax = prominence, None
        if isinstance(pmin, np.ndarray) or isinstance(pmax, np.ndarray):
            raise NotImplementedError("per-sample (array-valued) prominence intervals are not supported")
    nan = float("nan")
    return (0.0 if distance is None else float(distance),
            nan if pmin is None else float(pmin), nan if pmax is None else float(pmax))


def phase_correlate_args(src, tgt):
    """The argument checks of Context.phase_correlate, made before any device call -> (src, tgt) as arrays.  Different shapes:
    AssertionError (the reference's assert); neither a 2-D image nor a 3-D batch, or a side outside [2, 4096]: ValueError."""
    a, b = np.asarray(src), np.asarray(tgt)
    assert a.shape == b.shape, "Images need to have the same shape!"
    if a.ndim not in (2, 3):
        raise ValueError(f"phase_correlate: two 2-D images or two 3-D batches, not {a.ndim}-D")
    if a.ndim == 3 and a.shape[0] < 1:
        raise ValueError("phase_correlate: an empty batch")
    rows, cols = a.shape[-2:]
    if not (2 <= rows <= PHASE_CORRELATE_MAX and 2 <= cols <= PHASE_CORRELATE_MAX):
        raise ValueError(f"phase_correlate: image sides in [2, {PHASE_CORRELATE_MAX}], not {rows} x {cols}")
    return a, b


def fmt_clip_radius(cols, clip_px, downsample, rows):
    """The range clip and the width after the resize of the batched rotation prior -> (clip, R), checked as the library checks them:
    ValueError for rows outside [8, 16384], downsample < 1, or R = clip // downsample outside [4, 1303] (round(pi R) must fit the
    FFT's 4096)."""
    clip_px, downsample = int(clip_px), int(downsample)
    if not 8 <= rows <= FMT_MAX_ROWS:
        raise ValueError(f"fmt_rotation_batch: polar images of 8 to {FMT_MAX_ROWS} rows, not {rows}")
    if downsample < 1:
        raise ValueError(f"fmt_rotation_batch: downsample >= 1, not {downsample}")
    clip = clip_px if 0 < clip_px < cols else cols
    R = clip // downsample
    if not FMT_MIN_R <= R <= FMT_MAX_R:
        raise ValueError(f"fmt_rotation_batch: clip // downsample in [{FMT_MIN_R}, {FMT_MAX_R}], not {clip} // {downsample} = {R}")
    return clip, R


def fmt_rotation_batch_args(src, tgt, clip_px, downsample):
    """The argument checks of Context.fmt_rotation_batch, made before any device call -> (src, tgt as arrays, clip, R).  Different
    shapes: AssertionError (the reference's assert); neither 2-D images nor 3-D batches, an empty batch, or fmt_clip_radius's
    conditions: ValueError."""
    a, b = np.asarray(src), np.asarray(tgt)
    assert a.shape == b.shape, "Images need to have the same shape!"
    if a.ndim not in (2, 3):
        raise ValueError(f"fmt_rotation_batch: two 2-D polar images or two 3-D batches, not {a.ndim}-D")
    if a.ndim == 3 and a.shape[0] < 1:
        raise ValueError("fmt_rotation_batch: an empty batch")
    rows, cols = a.shape[-2:]
    if cols < 2:
        raise ValueError(f"fmt_rotation_batch: at least 2 columns, not {cols}")
    clip, R = fmt_clip_radius(cols, clip_px, downsample, rows)
    return a, b, clip, R


def fmt_cart_radius(cols, cart_downsample):
    """The Cartesian half of the registration: Rc = cols // cart_downsample, checked as the library checks it.  TypeError for a
    cart_downsample that is no integer (as convertPolarImageToCartesian); ValueError for one below 1, for more than 16384 columns,
    or for a side 2 Rc outside [2, 4096], the phase correlation's limit."""
    if not isinstance(cart_downsample, numbers.Integral):
        raise TypeError(f"fmt_register: cart_downsample must be an integer, not {type(cart_downsample).__name__}")
    cart_downsample = int(cart_downsample)
    if cart_downsample < 1:
        raise ValueError(f"fmt_register: cart_downsample >= 1, not {cart_downsample}")
    if cols > FMT_MAX_COLS:
        raise ValueError(f"fmt_register: at most {FMT_MAX_COLS} columns, not {cols}")
    Rc = cols // cart_downsample
    if not 2 <= 2 * Rc <= PHASE_CORRELATE_MAX:
        raise ValueError(f"fmt_register: a Cartesian side 2 * (cols // cart_downsample) in [2, {PHASE_CORRELATE_MAX}], not "
                         f"2 * ({cols} // {cart_downsample}) = {2 * Rc}")
    return Rc


def fmt_register_batch_args(src, tgt, clip_px, downsample, cart_downsample):
    """The argument checks of Context.fmt_register_batch, made before any device call -> (src, tgt as arrays, clip, R, Rc):
    fmt_rotation_batch_args's (AssertionError for different shapes, else ValueError), then fmt_cart_radius's."""
    a, b, clip, R = fmt_rotation_batch_args(src, tgt, clip_px, downsample)
    return a, b, clip, R, fmt_cart_radius(a.shape[-1], cart_downsample)


def invert_affine(M):
    """cv2.warpAffine's in-place inversion of a 2 x 3 matrix, operation by operation in float64 (a singular matrix -> all zeros)
    -> the six coefficients of the destination -> source map"""
    M0, M1, M2, M3, M4, M5 = (float(v) for v in np.asarray(M, np.float64).ravel())
    D = M0 * M4 - M1 * M3
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M4 * D, M0 * D
    M0, M1, M3, M4 = A11, M1 * -D, M3 * -D, A22
    b1 = -M0 * M2 - M1 * M5
    b2 = -M3 * M2 - M4 * M5
    return np.array([M0, M1, b1, M3, M4, b2], np.float64)


def warp_affine_args(src, M, dsize_wh, inverse_map=False):
    """The argument checks of Context.warp_affine_f32, made before any device call -> (src as an array, M as (m_count, 6) float64,
    dw, dh).  ValueError: src neither a 2-D image nor a 3-D batch; M not (2, 3) or (n, 2, 3) (a stack of matrices needs a batch of as
    many images); a non-finite M; an empty source or output; a side above 16384; a map that sends any of the four corners of
    the destination to a source coordinate of magnitude >= 2^20 px (or to no finite one), evaluated in float64 with the inverted
    matrix."""
    a = np.asarray(src)
    if a.ndim not in (2, 3):
        raise ValueError(f"warp_affine_f32: a 2-D image or a 3-D batch, not {a.ndim}-D")
    m = np.asarray(M, np.float64)
    if m.shape != (2, 3) and not (a.ndim == 3 and m.shape == (a.shape[0], 2, 3)):
        raise ValueError(f"warp_affine_f32: M of shape (2, 3){' or (%d, 2, 3)' % a.shape[0] if a.ndim == 3 else ''}, not {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError("warp_affine_f32: M is not finite")
    dw, dh = int(dsize_wh[0]), int(dsize_wh[1])
    if min(dw, dh) <= 0 or min(a.shape) <= 0:
        raise ValueError(f"warp_affine_f32: empty image ({a.shape} -> {dh} x {dw})")
    if max(dw, dh, a.shape[-2], a.shape[-1]) > WARP_AFFINE_MAX_SIDE:
        raise ValueError(f"warp_affine_f32: image side above {WARP_AFFINE_MAX_SIDE} ({a.shape[-2]} x {a.shape[-1]} -> {dh} x {dw})")
    m = np.ascontiguousarray(m.reshape(-1, 6))
    for k in range(len(m)):
        inv = m[k] if inverse_map else invert_affine(m[k])
        inv = [float(v) for v in inv]
        worst = max(abs(inv[r] * x + inv[r + 1] * y + inv[r + 2]) for r in (0, 3) for x in (0, dw - 1) for y in (0, dh - 1))
        if not worst < WARP_AFFINE_MAX_COORD:
            raise ValueError(f"warp_affine_f32: matrix {k} maps a corner of the output to source coordinate {worst:g} px; the "
                             f"fixed-point coordinates hold magnitudes below 2^20 px")
    return a, m, dw, dh


KLT_MAX_GUESS = float(1 << 20)          # ROAM_KLT_MAX_GUESS
PRIOR_MAX_LINEAR = 64.0                 # ROAM_PRIOR_MAX_LINEAR


def klt_flow_args(pts, init_pts):
    """The argument checks of Context.klt_track's initial flow, made before any device call -> (pts (K, 2) float32, init_pts (K, 2)
    float32 or None).  ValueError: init_pts whose shape is not that of pts, a guess that is not finite, or one beyond
    KLT_MAX_GUESS = 2^20 px in magnitude (what roam_klt_track_*_flow refuse)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    if init_pts is None:
        return pts, None
    g = np.asarray(init_pts)
    if g.shape != pts.shape:
        raise ValueError(f"klt_track: init_pts of shape {pts.shape} like pts, not {g.shape}")
    g = np.ascontiguousarray(g, np.float32)
    if not np.isfinite(g).all():
        raise ValueError("klt_track: init_pts is not finite")
    if g.size and float(np.abs(g).max()) > KLT_MAX_GUESS:
        raise ValueError(f"klt_track: init_pts beyond 2^20 px in magnitude ({float(np.abs(g).max()):g})")
    return pts, g


def motion_prior_args(affine, use, lanes):
    """The argument checks of Engine.set_motion_prior, made before any device call -> (affine (lanes, 6) float32, use (lanes,) uint8 or
    None).  ValueError: affine neither (lanes, 2, 3) nor (lanes, 6), use not (lanes,), an entry that is not finite, a linear coefficient
    above PRIOR_MAX_LINEAR = 64 or a translation above KLT_MAX_GUESS = 2^20 px in magnitude (what roam_engine_set_motion_prior refuses)."""
    a = np.asarray(affine)
    if a.shape not in ((lanes, 2, 3), (lanes, 6)):
        raise ValueError(f"set_motion_prior: affine of shape ({lanes}, 2, 3) or ({lanes}, 6), not {a.shape}")
    a = np.ascontiguousarray(a.reshape(lanes, 6), np.float32)
    if not np.isfinite(a).all():
        raise ValueError("set_motion_prior: affine is not finite")
    if float(np.abs(a[:, [0, 1, 3, 4]]).max()) > PRIOR_MAX_LINEAR or float(np.abs(a[:, [2, 5]]).max()) > KLT_MAX_GUESS:
        raise ValueError(f"set_motion_prior: linear coefficients within {PRIOR_MAX_LINEAR:g}, translations within 2^20 px")
    if use is not None:
        u = np.asarray(use)
        if u.shape != (lanes,):
            raise ValueError(f"set_motion_prior: use of shape ({lanes},), not {u.shape}")
        use = np.ascontiguousarray(u != 0, np.uint8)
    return a, use


def auto_prior_args(cols, rows, clip_px, downsample, cart_downsample, min_rot_response, min_trans_response):
    """The argument checks of Engine.set_auto_prior, made before any device call -> AutoPriorCfg.  cols, rows: the engine's clip and
    rows.  What Engine.fmt_register refuses - fmt_clip_radius's and fmt_cart_radius's conditions: ValueError, TypeError for a
    cart_downsample that is no integer - and a response minimum that is negative or not finite: ValueError."""
    fmt_clip_radius(cols, clip_px, downsample, rows)
    fmt_cart_radius(cols, cart_downsample)
    gates = []
    for name, v in (("min_rot_response", min_rot_response), ("min_trans_response", min_trans_response)):
        v = float(v)
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f"set_auto_prior: {name} finite and >= 0, not {v}")
        gates.append(v)
    clip_px, downsample, cart_downsample = int(clip_px), int(downsample), int(cart_downsample)
    if clip_px == 0 and downsample == 0 and cart_downsample == 0:        # (refused above: downsample < 1; never the ABI's "defaults")
        raise ValueError("set_auto_prior: downsample >= 1")
    return AutoPriorCfg(clip_px, downsample, cart_downsample, gates[0], gates[1])


def pose_graph_args(graphs, max_iterations=20, max_trials=10, lambda_init=0.0):
    """The argument checks of Context.pose_graph_optimize and pose_graph_plan, made before any library call -> (vertex_off, poses,
    fixed, edge_off, edge_ij, meas, info6, huber or None, PoseGraphOpts): the graphs packed as roam_pose_graph_optimize takes them.
    graphs: a list of (poses (V, 3), fixed (V,), edge_ij (E, 2), meas (E, 3), info (E, 3, 3) or (3, 3), huber (E,) or None).
    ValueError: wrong shapes, an information matrix that is not exactly symmetric, and everything the ABI refuses - no graph or more
    than 65535, a graph with no vertex or more than 32768, an edge index out of range or i == j, a pose / measurement / information
    entry / Huber width that is not finite, a negative Huber width, a graph without a fixed vertex, options out of range."""
    graphs = list(graphs)
    if not 1 <= len(graphs) <= POSE_GRAPH_MAX_GRAPHS:
        raise ValueError(f"pose_graph: 1 to {POSE_GRAPH_MAX_GRAPHS} graphs, not {len(graphs)}")
    max_iterations, max_trials, lambda_init = int(max_iterations), int(max_trials), float(lambda_init)
    if not 0 <= max_iterations <= POSE_GRAPH_MAX_ITERATIONS:
        raise ValueError(f"pose_graph: max_iterations in [0, {POSE_GRAPH_MAX_ITERATIONS}], not {max_iterations}")
    if not 0 <= max_trials <= POSE_GRAPH_MAX_TRIALS:
        raise ValueError(f"pose_graph: max_trials in [0, {POSE_GRAPH_MAX_TRIALS}], not {max_trials}")
    if not (np.isfinite(lambda_init) and lambda_init >= 0.0):
        raise ValueError(f"pose_graph: lambda_init finite and >= 0, not {lambda_init}")
    P, Fx, IJ, Z, O, Hb = [], [], [], [], [], []
    any_huber = False
    for g, graph in enumerate(graphs):
        if len(graph) != 6:
            raise ValueError(f"pose_graph: graph {g} is (poses, fixed, edge_ij, meas, info, huber), not {len(graph)} items")
        poses, fixed, ij, meas, info, huber = graph
        poses, fixed = np.asarray(poses, np.float64), np.asarray(fixed)
        if poses.ndim != 2 or poses.shape[1] != 3 or fixed.shape != (poses.shape[0],):
            raise ValueError(f"pose_graph: graph {g}: poses (V, 3) and fixed (V,), not {poses.shape} and {fixed.shape}")
        V = poses.shape[0]
        if not 1 <= V <= POSE_GRAPH_MAX_VERTICES:
            raise ValueError(f"pose_graph: graph {g}: 1 to {POSE_GRAPH_MAX_VERTICES} vertices, not {V}")
        if not np.isfinite(poses).all():
            raise ValueError(f"pose_graph: graph {g}: a pose that is not finite")
        fixed = fixed != 0
        if not fixed.any():
            raise ValueError(f"pose_graph: graph {g} has no fixed vertex")
        ij = np.asarray(ij)
        if ij.size == 0:                    # no edges, however the caller wrote that ([] is a float64 array)
            ij = np.zeros((0, 2), np.int32)
        if ij.ndim != 2 or ij.shape[1] != 2 or ij.dtype.kind not in "iu":
            raise ValueError(f"pose_graph: graph {g}: edge_ij (E, 2) of integers, not {ij.dtype} {ij.shape}")
        E = ij.shape[0]
        meas = np.asarray(meas, np.float64)
        meas = meas.reshape(0, 3) if meas.size == 0 else meas
        if meas.shape != (E, 3):
            raise ValueError(f"pose_graph: graph {g}: meas ({E}, 3), not {meas.shape}")
        info = np.asarray(info, np.float64)
        if info.shape == (3, 3):
            info = np.broadcast_to(info, (E, 3, 3))
        elif info.size == 0 and E == 0:
            info = np.zeros((0, 3, 3))
        if info.shape != (E, 3, 3):
            raise ValueError(f"pose_graph: graph {g}: info ({E}, 3, 3) or (3, 3), not {info.shape}")
        bad = np.flatnonzero(((ij < 0) | (ij >= V)).any(axis=1) | (ij[:, 0] == ij[:, 1]))
        if bad.size:
            t = int(bad[0])
            raise ValueError(f"pose_graph: graph {g}, edge {t}: vertices ({int(ij[t, 0])}, {int(ij[t, 1])}) - two different indices in [0, {V})")
        bad = np.flatnonzero(~(np.isfinite(meas).all(axis=1) & np.isfinite(info).all(axis=(1, 2))))
        if bad.size:
            raise ValueError(f"pose_graph: graph {g}, edge {int(bad[0])}: a measurement or information entry that is not finite")
        bad = np.flatnonzero((info != info.transpose(0, 2, 1)).any(axis=(1, 2)))
        if bad.size:
            raise ValueError(f"pose_graph: graph {g}, edge {int(bad[0])}: the information matrix is not exactly symmetric")
        if huber is None:
            hb = np.zeros(E)
        else:
            any_huber = True
            hb = np.asarray(huber, np.float64)
            if hb.shape != (E,):
                raise ValueError(f"pose_graph: graph {g}: huber ({E},) or None, not {hb.shape}")
            bad = np.flatnonzero(~(np.isfinite(hb) & (hb >= 0.0)))
            if bad.size:
                raise ValueError(f"pose_graph: graph {g}, edge {int(bad[0])}: a Huber width that is negative or not finite")
        P.append(poses)
        Fx.append(fixed.astype(np.uint8))
        IJ.append(ij.astype(np.int32))
        Z.append(meas)
        O.append(info.reshape(E, 9)[:, [0, 1, 2, 4, 5, 8]])
        Hb.append(hb)
    vertex_off = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(np.int32)
    edge_off = np.concatenate([[0], np.cumsum([len(e) for e in IJ])]).astype(np.int32)
    return (vertex_off, np.ascontiguousarray(np.concatenate(P), np.float64), np.ascontiguousarray(np.concatenate(Fx)), edge_off,
            np.ascontiguousarray(np.concatenate(IJ).reshape(-1, 2)), np.ascontiguousarray(np.concatenate(Z).reshape(-1, 3)),
            np.ascontiguousarray(np.concatenate(O).reshape(-1, 6)), np.ascontiguousarray(np.concatenate(Hb)) if any_huber else None,
            PoseGraphOpts(max_iterations, max_trials, lambda_init))


def pose_graph_plan(graphs):
    """roam_pose_graph_plan, host code only (no device, no context): the envelope of every graph in 3 x 3 blocks and the device
    scratch (bytes) of the call's largest chunk -> (envelope_blocks (n,) int64, scratch_bytes).  There is no reordering: block row k
    of the system runs from the lowest-numbered free neighbour of free vertex k to the diagonal, so a graph costs about its vertex
    count plus the sum of j - i over its non-consecutive edges, 144 bytes per block.  ValueError: pose_graph_args's conditions, and a
    single graph whose scratch exceeds a chunk of 2000 MiB."""
    vertex_off, _, fixed, edge_off, ij, _, _, _, _ = pose_graph_args(graphs)
    env = np.zeros(len(vertex_off) - 1, np.int64)
    nbytes = C.c_int64(0)
    rc = load_library().roam_pose_graph_plan(len(env), _ptr(vertex_off), _ptr(fixed), _ptr(edge_off), _ptr(ij), _ptr(env), C.byref(nbytes))
    if rc != ROAM_OK:
        # pose_graph_args has passed, so what the host half refuses is a graph too large for a launch; it has no context to leave a
        # text in: find the graph here (one call each) and state its envelope as roam_pose_graph_optimize's text does
        for g in range(len(env)):
            v0, e0, e1 = vertex_off[g], edge_off[g], edge_off[g + 1]
            one_v, one_e = np.array([0, vertex_off[g + 1] - v0], np.int32), np.array([0, e1 - e0], np.int32)
            f, e = np.ascontiguousarray(fixed[v0:vertex_off[g + 1]]), np.ascontiguousarray(ij[e0:e1])
            if load_library().roam_pose_graph_plan(1, _ptr(one_v), _ptr(f), _ptr(one_e), _ptr(e), None, None) != ROAM_OK:
                cidx = np.cumsum(f == 0) - 1
                a, b = cidx[e[:, 0]], cidx[e[:, 1]]
                both = (f[e[:, 0]] == 0) & (f[e[:, 1]] == 0)
                first = np.arange(int((f == 0).sum()))
                np.minimum.at(first, np.maximum(a, b)[both], np.minimum(a, b)[both])
                blocks = int((np.arange(len(first)) - first + 1).sum())
                raise ValueError(f"pose_graph: graph {g}: an envelope of {blocks} blocks ({144 * blocks} bytes of matrix) needs more than "
                                 f"the {POSE_GRAPH_CHUNK_BYTES} bytes of device scratch of a launch (no reordering: the envelope is "
                                 "the vertex count plus the span of every loop edge)")
        raise ValueError("pose_graph: roam_pose_graph_plan refused the graphs")
    return env, int(nbytes.value)


def scan_context_plan(rows, cols, clip_px, sectors, rings):
    """roam_scan_context_plan, host code only (no device, no context): the argument checks of the describing entries and the bin
    edges -> (clip, row_edges (S + 1,), col_edges (R + 1,)) int32.  Sector s covers the rows [row_edges[s], row_edges[s + 1]), ring r
    the columns [col_edges[r], col_edges[r + 1]); clip = clip_px if 0 < clip_px < cols else cols.  ValueError: sectors outside [2, 256],
    rings outside [1, 128], rows < sectors or > 65536, clip < rings or > 4096, or anything that is no integer."""
    for name, v in (("rows", rows), ("cols", cols), ("sectors", sectors), ("rings", rings)):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool):
            raise ValueError(f"scan context: {name} is an integer, not {v!r}")
    if clip_px is not None and (not isinstance(clip_px, numbers.Integral) or isinstance(clip_px, bool)):
        raise ValueError(f"scan context: clip_px is an integer or None, not {clip_px!r}")
    if not 2 <= sectors <= SCAN_CONTEXT_MAX_SECTORS:
        raise ValueError(f"scan context: sectors in [2, {SCAN_CONTEXT_MAX_SECTORS}], not {sectors}")
    if not 1 <= rings <= SCAN_CONTEXT_MAX_RINGS:
        raise ValueError(f"scan context: rings in [1, {SCAN_CONTEXT_MAX_RINGS}], not {rings}")
    if not sectors <= rows <= SCAN_CONTEXT_MAX_ROWS:
        raise ValueError(f"scan context: rows in [sectors = {sectors}, {SCAN_CONTEXT_MAX_ROWS}], not {rows}")
    if not 1 <= cols < 2 ** 31:
        raise ValueError(f"scan context: cols >= 1, not {cols}")
    clip = int(clip_px) if clip_px is not None and 0 < clip_px < cols else int(cols)
    if not rings <= clip <= SCAN_CONTEXT_MAX_CLIP:
        raise ValueError(f"scan context: clip_px (the range bins kept) in [rings = {rings}, {SCAN_CONTEXT_MAX_CLIP}], not {clip}")
    re, ce = np.empty(sectors + 1, np.int32), np.empty(rings + 1, np.int32)
    rc = load_library().roam_scan_context_plan(int(rows), int(cols), clip, int(sectors), int(rings), _ptr(re), _ptr(ce))
    if rc != ROAM_OK:
        raise ValueError(f"scan context: roam_scan_context_plan refused rows {rows}, cols {cols}, clip_px {clip_px}, {sectors} x {rings}")
    return clip, re, ce


def scan_context_floor(floor):
    """the float floor of the describing entries: finite and >= 0 (ValueError otherwise)"""
    if not isinstance(floor, numbers.Real) or isinstance(floor, bool) or not np.isfinite(floor) or floor < 0:
        raise ValueError(f"scan context: floor finite and >= 0, not {floor!r}")
    return float(floor)


def scan_context_images(polar, clip_px, sectors, rings):
    """the image operand of the describing entries -> (a3, n, rows, cols, row_stride, image_stride, clip): a 2-D image or a 3-D batch
    of float32, read in place where its strides allow (_f32_rows_in_place).  ValueError as scan_context_plan"""
    a = np.asarray(polar)
    if a.ndim not in (2, 3) or a.size == 0:
        raise ValueError(f"scan context: a 2-D image or a 3-D batch, not shape {a.shape}")
    a = _f32_rows_in_place(a)
    a3 = a if a.ndim == 3 else a[None]
    n, rows, cols = a3.shape
    clip, _, _ = scan_context_plan(rows, cols, clip_px, sectors, rings)
    row_stride = a3.strides[1] // 4
    image_stride = a3.strides[0] // 4 if n > 1 else rows * row_stride
    return a3, n, rows, cols, row_stride, image_stride, clip


def loop_query_args(count, indices, max_index, k, max_distance):
    """the checks of LoopDb.query before any library call -> (query_index, max_index) int32 arrays"""
    q = np.ascontiguousarray(indices, np.int32).ravel()
    m = np.ascontiguousarray(max_index, np.int32).ravel()
    if len(q) < 1 or len(q) != len(m):
        raise ValueError(f"loop query: query indices and max_index of one length >= 1, not {len(q)} and {len(m)}")
    if q.min() < 0 or q.max() >= count:
        raise ValueError(f"loop query: query indices in [0, {count})")
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 1 <= k <= LOOP_MAX_K:
        raise ValueError(f"loop query: k in [1, {LOOP_MAX_K}], not {k!r}")
    if not isinstance(max_distance, numbers.Real) or np.isnan(max_distance):
        raise ValueError(f"loop query: max_distance is a number, not {max_distance!r}")
    return q, m


def loop_offsets_args(offsets_m, range_resolution_m, capacity=None, sectors=None, rings=None):
    """the checks of LoopDb.keep_offsets and Context.scan_context_offsets before any library call -> (offsets (n, 2) float64, C order,
    range_resolution_m).  ValueError: not (n, 2) numbers with 1 <= n <= 48, an offset that is not finite, beyond 1e6 m or (0, 0), a
    resolution that is not finite or <= 0, a variant store (capacity x n x sectors x (4 rings + 8 padded rings + 4) bytes) beyond 2000 MiB"""
    a = np.asarray(offsets_m)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"scan context offsets: offsets of numbers, not {a.dtype}")
    if a.ndim == 1 and a.size == 2:
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2 or not 1 <= len(a) <= LOOP_MAX_OFFSETS:
        raise ValueError(f"scan context offsets: (n, 2) offsets in metres with 1 <= n <= {LOOP_MAX_OFFSETS}, not shape {a.shape}")
    a = np.ascontiguousarray(a, np.float64)
    if not np.all(np.abs(a) <= ICP_MAX_COORD):
        raise ValueError(f"scan context offsets: an offset that is not finite or beyond {ICP_MAX_COORD:g} m")
    if np.any(np.all(a == 0.0, axis=1)):
        raise ValueError("scan context offsets: the offset (0, 0) - variant 0 is the plain descriptor already")
    res = range_resolution_m
    if not isinstance(res, numbers.Real) or isinstance(res, bool) or not np.isfinite(res) or not res > 0:
        raise ValueError(f"scan context offsets: range_resolution_m finite and > 0, not {res!r}")
    if capacity is not None:
        per = len(a) * sectors * (4 * rings + 8 * ((rings + 3) & ~3) + 4)
        if capacity * per > LOOP_DB_BYTES:
            raise ValueError(f"loop db: capacity {capacity} x {len(a)} offsets x {per // len(a)} bytes is beyond the {LOOP_DB_BYTES} bytes of a variant store")
    return a, float(res)


def scan_context_offset_table(rows, sectors):
    """roam_scan_context_offset_table, host code only (no device, no context): the tables of the origin-shifted descriptor by the
    host's libm -> (cos, sin of the row centres (rows,), cos, sin of the sector boundaries (sectors,)) float64.  ValueError outside
    scan_context_plan's limits"""
    for name, v in (("rows", rows), ("sectors", sectors)):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool):
            raise ValueError(f"scan context: {name} is an integer, not {v!r}")
    if not 2 <= sectors <= SCAN_CONTEXT_MAX_SECTORS or not sectors <= rows <= SCAN_CONTEXT_MAX_ROWS:
        raise ValueError(f"scan context: sectors in [2, {SCAN_CONTEXT_MAX_SECTORS}] and rows in [sectors, {SCAN_CONTEXT_MAX_ROWS}], not {sectors} and {rows}")
    out = [np.empty(rows), np.empty(rows), np.empty(sectors), np.empty(sectors)]
    if load_library().roam_scan_context_offset_table(int(rows), int(sectors), *[_ptr(a) for a in out]) != ROAM_OK:
        raise ValueError(f"scan context: roam_scan_context_offset_table refused rows {rows}, sectors {sectors}")
    return tuple(out)


def polar_cloud_table(rows):
    """roam_polar_cloud_table, host code only (no device, no context): (cos, sin) float64 of phi_t = (2 pi t) / rows, t < rows, by the
    host's libm - the table a cloud-keeping loop database multiplies with.  ValueError: rows no integer in [1, 65536]"""
    if not isinstance(rows, numbers.Integral) or isinstance(rows, bool) or not 1 <= rows <= SCAN_CONTEXT_MAX_ROWS:
        raise ValueError(f"loop db: rows an integer in [1, {SCAN_CONTEXT_MAX_ROWS}], not {rows!r}")
    c, s = np.empty(rows, np.float64), np.empty(rows, np.float64)
    if load_library().roam_polar_cloud_table(int(rows), _ptr(c), _ptr(s)) != ROAM_OK:
        raise ValueError(f"loop db: roam_polar_cloud_table refused rows {rows}")
    return c, s


def loop_cloud_args(capacity, rows, max_points, point_stride, range_resolution_m):
    """the checks of LoopDb.keep_clouds before any library call -> (rows, max_points, point_stride, range_resolution_m)"""
    if not isinstance(rows, numbers.Integral) or isinstance(rows, bool) or not 1 <= rows <= SCAN_CONTEXT_MAX_ROWS:
        raise ValueError(f"loop db: rows an integer in [1, {SCAN_CONTEXT_MAX_ROWS}], not {rows!r}")
    if not isinstance(max_points, numbers.Integral) or isinstance(max_points, bool) or not 1 <= max_points <= ICP_MAX_POINTS:
        raise ValueError(f"loop db: max_points an integer in [1, {ICP_MAX_POINTS}], not {max_points!r}")
    if not isinstance(point_stride, numbers.Integral) or isinstance(point_stride, bool) or not 1 <= point_stride < 2 ** 31:
        raise ValueError(f"loop db: point_stride an integer >= 1, not {point_stride!r}")
    res = range_resolution_m
    if not isinstance(res, numbers.Real) or isinstance(res, bool) or not np.isfinite(res) or not res > 0:
        raise ValueError(f"loop db: range_resolution_m finite and > 0, not {res!r}")
    if capacity * max_points * 16 > LOOP_DB_BYTES:
        raise ValueError(f"loop db: capacity {capacity} x max_points {max_points} x 16 bytes is beyond the {LOOP_DB_BYTES} bytes of a database")
    return int(rows), int(max_points), int(point_stride), float(res)


def loop_cloud_points(xy, max_points):
    """a cloud for LoopDb.set_cloud -> (n, 2) float64, C order.  ValueError: not (n, 2) numbers, n > max_points, a coordinate that is not
    finite or beyond 1e6 m"""
    a = np.asarray(xy)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"loop db: a cloud of numbers, not {a.dtype}")
    if a.size == 0 and a.ndim <= 2:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"loop db: a cloud (n, 2), not {a.shape}")
    if len(a) > max_points:
        raise ValueError(f"loop db: a cloud of {len(a)} points, more than max_points = {max_points}")
    a = np.ascontiguousarray(a, np.float64)
    if not np.all(np.abs(a) <= ICP_MAX_COORD):
        raise ValueError(f"loop db: a coordinate that is not finite or beyond {ICP_MAX_COORD:g} m")
    return a


def loop_verify_args(count, src_index, dst_index, init):
    """the checks of LoopDb.verify before any library call -> (src_index, dst_index int32, init (n, 3) float64)"""
    si = np.ascontiguousarray(src_index, np.int32).ravel()
    di = np.ascontiguousarray(dst_index, np.int32).ravel()
    if not 1 <= len(si) <= ICP_MAX_PAIRS or len(si) != len(di):
        raise ValueError(f"loop verify: src_index and dst_index of one length in [1, {ICP_MAX_PAIRS}], not {len(si)} and {len(di)}")
    if min(si.min(), di.min()) < 0 or max(si.max(), di.max()) >= count:
        raise ValueError(f"loop verify: entry indices in [0, {count})")
    x0 = np.zeros((len(si), 3)) if init is None else np.asarray(init, np.float64)
    if x0.shape == (3,):
        x0 = np.tile(x0, (len(si), 1))
    if x0.shape != (len(si), 3):
        raise ValueError(f"loop verify: init (3,) or ({len(si)}, 3) rows (theta, tx, ty), not {x0.shape}")
    if not (np.all(np.isfinite(x0)) and np.all(np.abs(x0[:, 1:]) <= ICP_MAX_COORD)):
        raise ValueError(f"loop verify: an initial pose that is not finite or beyond {ICP_MAX_COORD:g} m")
    return si, di, np.ascontiguousarray(x0)


def map_pose_table(poses):
    """roam_map_pose_table, host code only (no device, no context): poses (n, 3) rows x, y, theta -> (n, 2) float64 rows (cos theta,
    sin theta) by the host's libm - the values a global map's kernels multiply with.  ValueError: not (n, 3), a theta that is not finite"""
    p = np.ascontiguousarray(poses, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"global map: poses (n, 3) rows x, y, theta, not {p.shape}")
    cs = np.empty((len(p), 2), np.float64)
    if load_library().roam_map_pose_table(len(p), _ptr(p), _ptr(cs)) != ROAM_OK:
        raise ValueError("global map: poses with a theta that is not finite")
    return cs


def map_plan(bounds, res):
    """roam_map_plan, host code only: bounds (min x, max x, min y, max y) metres and the cell size -> (ox, oy, W, H), the extent with one
    cell of margin on each side.  ValueError: bounds that are not finite or min > max, res not finite or <= 0, a cell too fine for the
    coordinates, more than MAP_MAX_CELLS cells"""
    b = np.asarray(bounds, np.float64).ravel()
    if b.shape != (4,):
        raise ValueError(f"global map: bounds (min x, max x, min y, max y), not shape {np.shape(bounds)}")
    if not isinstance(res, numbers.Real) or isinstance(res, bool):
        raise ValueError(f"global map: res finite and > 0, not {res!r}")
    ox, oy, W, H = C.c_double(0), C.c_double(0), C.c_int32(0), C.c_int32(0)
    rc = load_library().roam_map_plan(b[0], b[1], b[2], b[3], float(res), C.byref(ox), C.byref(oy), C.byref(W), C.byref(H))
    if rc == ROAM_E_CAPACITY:
        raise ValueError(f"global map: bounds {b.tolist()} at res {res} take more than W H = {MAP_MAX_CELLS} cells")
    if rc != ROAM_OK:
        raise ValueError(f"global map: finite bounds with min <= max and a res finite, > 0 and not below 2^-50 of them, not {b.tolist()} and {res!r}")
    return ox.value, oy.value, W.value, H.value


def loop_map_args(count, poses, use=None, res=0.5, extent=None, min_hits=1, min_views=1):
    """the checks of LoopDb.map_bounds / map_render before any library call -> (poses (count, 3) float64, use (count,) int8 or None,
    res, extent (ox, oy, W, H) or None, min_hits, min_views)"""
    p = np.asarray(poses)
    if p.dtype.kind not in "fiu":
        raise ValueError(f"global map: poses of numbers, not {p.dtype}")
    if p.size == 0 and count == 0:
        p = p.reshape(0, 3)
    if p.shape != (count, 3):
        raise ValueError(f"global map: poses ({count}, 3) rows x, y, theta - one per entry - not {p.shape}")
    p = np.ascontiguousarray(p, np.float64)
    if not (np.all(np.isfinite(p)) and np.all(np.abs(p[:, :2]) <= ICP_MAX_COORD)):
        raise ValueError(f"global map: poses with an entry that is not finite or beyond {ICP_MAX_COORD:g} m")
    if use is not None:
        u = np.asarray(use)
        if u.dtype.kind not in "biu" or u.shape != (count,):
            raise ValueError(f"global map: use ({count},) flags - one per entry - not {u.dtype} {u.shape}")
        use = np.ascontiguousarray(u != 0, np.int8)
    if not isinstance(res, numbers.Real) or isinstance(res, bool) or not np.isfinite(res) or not res > 0:
        raise ValueError(f"global map: res finite and > 0, not {res!r}")
    if extent is not None:
        if len(extent) != 4:
            raise ValueError(f"global map: extent (ox, oy, W, H), not {extent!r}")
        ox, oy, W, H = extent
        if not all(isinstance(v, numbers.Real) and not isinstance(v, bool) and np.isfinite(v) for v in (ox, oy)):
            raise ValueError(f"global map: extent origin ox, oy finite, not {ox!r}, {oy!r}")
        if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 1 for v in (W, H)):
            raise ValueError(f"global map: extent W and H integers >= 1, not {W!r} and {H!r}")
        if W * H > MAP_MAX_CELLS:
            raise ValueError(f"global map: extent W H = {W * H} cells, more than {MAP_MAX_CELLS}")
        extent = (float(ox), float(oy), int(W), int(H))
    for name, v in (("min_hits", min_hits), ("min_views", min_views)):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or not 1 <= v < 2 ** 31:
            raise ValueError(f"global map: {name} an integer >= 1, not {v!r}")
    return p, use, float(res), extent, int(min_hits), int(min_views)


def icp2d_opts(opts=None):
    """the options of roam_icp2d_batch: None, a dict over ICP_DEFAULTS or an IcpOpts -> IcpOpts, checked.  ValueError: an unknown
    name, gates not 0 < gate_end <= gate_start (<= 1e6 m), gate_decay outside (0, 1], max_iterations outside [1, 1000],
    min_pairs < 2, an eps that is negative or not a number"""
    if isinstance(opts, IcpOpts):
        o = {name: getattr(opts, name) for name, _ in IcpOpts._fields_}
    else:
        unknown = set(opts or ()) - set(ICP_DEFAULTS)
        if unknown:
            raise ValueError(f"icp2d: unknown option(s) {sorted(unknown)}; known: {sorted(ICP_DEFAULTS)}")
        o = dict(ICP_DEFAULTS, **(opts or {}))
    for name in ("max_iterations", "min_pairs"):
        if not isinstance(o[name], numbers.Integral) or isinstance(o[name], bool):
            raise ValueError(f"icp2d: {name} an integer, not {o[name]!r}")
    for name in ("gate_start", "gate_end", "gate_decay", "eps_trans", "eps_rot"):
        if not isinstance(o[name], numbers.Real) or isinstance(o[name], bool):
            raise ValueError(f"icp2d: {name} a number, not {o[name]!r}")
    if not (np.isfinite(o["gate_start"]) and 0.0 < o["gate_end"] <= o["gate_start"] <= ICP_MAX_COORD):
        raise ValueError(f"icp2d: gates 0 < gate_end <= gate_start <= {ICP_MAX_COORD:g}, not {o['gate_end']} and {o['gate_start']}")
    if not 0.0 < o["gate_decay"] <= 1.0:
        raise ValueError(f"icp2d: gate_decay in (0, 1], not {o['gate_decay']}")
    if not 1 <= o["max_iterations"] <= ICP_ITERATION_LIMIT:
        raise ValueError(f"icp2d: max_iterations in [1, {ICP_ITERATION_LIMIT}], not {o['max_iterations']}")
    if o["min_pairs"] < 2 or o["min_pairs"] > 2 ** 31 - 1:
        raise ValueError(f"icp2d: min_pairs an int32 >= 2, not {o['min_pairs']}")
    if not (o["eps_trans"] >= 0.0 and o["eps_rot"] >= 0.0):
        raise ValueError(f"icp2d: eps_trans and eps_rot >= 0, not {o['eps_trans']} and {o['eps_rot']}")
    return IcpOpts(float(o["gate_start"]), float(o["gate_end"]), float(o["gate_decay"]), int(o["max_iterations"]), float(o["eps_trans"]),
                   float(o["eps_rot"]), int(o["min_pairs"]))


def icp2d_args(pairs, init=None, opts=None):
    """The argument checks of Context.icp2d_batch, made before a device is asked for -> (src_off, src, dst_off, dst, init, IcpOpts):
    the pairs packed as roam_icp2d_batch takes them.  pairs: a list of (src (n, 2), dst (m, 2)) in metres, n and m from 0 to 8192;
    init: (3,) for every pair or (len(pairs), 3) rows (theta, tx, ty), None = zeros; opts: see icp2d_opts.  ValueError: no pair or more
    than 65535, a cloud that is not (k, 2) or larger than the limit, a coordinate or pose that is not finite or beyond 1e6 m, an init
    of another shape, and what icp2d_opts refuses."""
    o = icp2d_opts(opts)
    pairs = list(pairs)
    if not 1 <= len(pairs) <= ICP_MAX_PAIRS:
        raise ValueError(f"icp2d: 1 to {ICP_MAX_PAIRS} pairs, not {len(pairs)}")
    S, D = [], []
    for p, pair in enumerate(pairs):
        if len(pair) != 2:
            raise ValueError(f"icp2d: pair {p} is (src, dst), not {len(pair)} items")
        for name, cloud, out in (("src", pair[0], S), ("dst", pair[1], D)):
            a = np.asarray(cloud)
            if a.dtype.kind not in "fiu":
                raise ValueError(f"icp2d: pair {p}: {name} of numbers, not {a.dtype}")
            a = a.astype(np.float64, copy=False)
            if a.size == 0 and a.ndim <= 2:
                a = a.reshape(0, 2)
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError(f"icp2d: pair {p}: {name} (k, 2), not {a.shape}")
            if len(a) > ICP_MAX_POINTS:
                raise ValueError(f"icp2d: pair {p}: {name} has {len(a)} points, more than {ICP_MAX_POINTS}")
            if not np.all(np.abs(a) <= ICP_MAX_COORD):              # NaN fails too
                raise ValueError(f"icp2d: pair {p}: {name} has a coordinate that is not finite or beyond {ICP_MAX_COORD:g} m")
            out.append(a)
    x0 = np.zeros((len(pairs), 3)) if init is None else np.asarray(init, np.float64)
    if x0.shape == (3,):
        x0 = np.tile(x0, (len(pairs), 1))
    if x0.shape != (len(pairs), 3):
        raise ValueError(f"icp2d: init (3,) or ({len(pairs)}, 3) rows (theta, tx, ty), not {x0.shape}")
    if not (np.all(np.isfinite(x0)) and np.all(np.abs(x0[:, 1:]) <= ICP_MAX_COORD)):
        raise ValueError(f"icp2d: an initial pose that is not finite or beyond {ICP_MAX_COORD:g} m")
    src_off = np.concatenate([[0], np.cumsum([len(a) for a in S])]).astype(np.int32)
    dst_off = np.concatenate([[0], np.cumsum([len(a) for a in D])]).astype(np.int32)
    return (src_off, np.ascontiguousarray(np.concatenate(S).reshape(-1, 2)), dst_off, np.ascontiguousarray(np.concatenate(D).reshape(-1, 2)),
            np.ascontiguousarray(x0), o)


def _f32_rows_in_place(a):
    """a float32 view with unit column stride and forward row / image strides is read in place; anything else is copied"""
    ok = a.dtype == np.float32 and a.strides[-1] == 4 and a.strides[-2] % 4 == 0 and a.strides[-2] >= 4 * a.shape[-1]
    if ok and a.ndim == 3:
        ok = a.strides[0] % 4 == 0 and a.strides[0] >= (a.shape[1] - 1) * a.strides[1] + 4 * a.shape[2]
    return a if ok else np.ascontiguousarray(a, np.float32)


def _batch_operands(a, b):
    """two images or two batches of one shape as the batched entries take them -> (a3, b3, n, rows, cols, row_stride, image_stride),
    strides in floats: _f32_rows_in_place on each, 2-D promoted to a batch of one"""
    a, b = _f32_rows_in_place(a), _f32_rows_in_place(b)
    a3, b3 = (a, b) if a.ndim == 3 else (a[None], b[None])
    n, rows, cols = a3.shape
    if a3.strides[0 if n > 1 else 1:] != b3.strides[0 if n > 1 else 1:]:     # one pair of strides describes both operands
        a3, b3 = np.ascontiguousarray(a3), np.ascontiguousarray(b3)
    row_stride = a3.strides[1] // 4
    image_stride = a3.strides[0] // 4 if n > 1 else rows * row_stride
    return a3, b3, n, rows, cols, row_stride, image_stride


_lib = None


def load_library():
    """dlopen libroam_hip.so and declare every signature of include/roam_abi.h."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RoamError(ROAM_E_NODEVICE, f"{LIB_PATH} not built - run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(LIB_PATH)
        partial = bool(os.environ.get("ROAM_LIB_PARTIAL"))      # a host-only build (profiles/asan_cpu.sh): the symbols it has
        for name, (res, args) in list(_SIGS.items()) + list(_INTERNAL_SIGS.items()):
            if partial and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)          # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


class Context:
    """One GPU + one HIP stream (roam_ctx).  Not thread-safe; make one per thread/GPU."""

    def __init__(self, device_id: int = 0):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.roam_create(int(device_id), C.byref(h))
        if rc != ROAM_OK:
            raise RoamError(rc, "roam_create failed: no usable MI355X/gfx950 device (the product path has no CPU fallback)")
        self.h = h
        self.device_id = device_id

    def close(self):
        if getattr(self, "h", None):
            self.lib.roam_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, ok=(ROAM_OK,)):
        if rc not in ok:
            raise RoamError(rc, self.lib.roam_last_error(self.h).decode(errors="replace"))
        return rc

    def device_info(self):
        name = C.create_string_buffer(256)
        arch = C.create_string_buffer(64)
        cu, mem = C.c_int32(0), C.c_int64(0)
        self.check(self.lib.roam_device_info(self.h, name, 256, C.byref(cu), C.byref(mem), arch, 64))
        return dict(name=name.value.decode(), arch=arch.value.decode(), cu_count=cu.value, hbm_bytes=mem.value)

    def host_alloc(self, shape, dtype=np.uint8):
        """numpy array backed by pinned host memory (freed with host_free)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = _vp()
        self.check(self.lib.roam_host_alloc(self.h, n, C.byref(p)))
        buf = (C.c_uint8 * n).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self.check(self.lib.roam_host_free(self.h, p))

    # ---- stage API -------------------------------------------------------------------
    def peaks_polar_f32(self, polar, distance=None, prominence=None):
        """distance / prominence: find_peaks' conditions (peak_conditions); None, None = the plain detection"""
        img = np.ascontiguousarray(polar, np.float32)
        rows, cols = img.shape
        cap = rows * ((cols + 1) // 2)
        out = np.empty((cap, 2), np.int32)
        n = C.c_int64(0)
        if distance is None and prominence is None:
            self.check(self.lib.roam_peaks_polar_f32(self.h, _ptr(img), rows, cols, _ptr(out), cap, C.byref(n)))
        else:
            d, pmin, pmax = peak_conditions(distance, prominence)
            self.check(self.lib.roam_peaks_polar_f32_cond(self.h, _ptr(img), rows, cols, d, pmin, pmax, _ptr(out), cap, C.byref(n)))
        return out[:n.value]

    def peaks_record_u8(self, rec, payload_off=11, clip=2025, distance=None, prominence=None):
        rec = np.ascontiguousarray(rec, np.uint8)
        rows, stride = rec.shape
        cap = rows * ((clip + 1) // 2)
        out = np.empty((cap, 2), np.int32)
        n = C.c_int64(0)
        if distance is None and prominence is None:
            self.check(self.lib.roam_peaks_record_u8(self.h, _ptr(rec), rows, stride, payload_off, clip, _ptr(out), cap, C.byref(n)))
        else:
            d, pmin, pmax = peak_conditions(distance, prominence)
            self.check(self.lib.roam_peaks_record_u8_cond(self.h, _ptr(rec), rows, stride, payload_off, clip, d, pmin, pmax, _ptr(out),
                                                          cap, C.byref(n)))
        return out[:n.value]

    def polar_to_cart_f32(self, polar, want_f32=True, want_u8=False):
        img = np.ascontiguousarray(polar, np.float32)
        rows, cols = img.shape
        W = 2 * (cols // 2)
        f = np.empty((W, W), np.float32) if want_f32 else None
        u = np.empty((W, W), np.uint8) if want_u8 else None
        self.check(self.lib.roam_polar_to_cart_f32(self.h, _ptr(img), rows, cols, _ptr(f), _ptr(u)))
        return f, u

    def polar_to_cart_record_u8(self, rec, payload_off=11, clip=2025, want_f32=False, want_u8=True):
        rec = np.ascontiguousarray(rec, np.uint8)
        rows, stride = rec.shape
        W = 2 * (clip // 2)
        f = np.empty((W, W), np.float32) if want_f32 else None
        u = np.empty((W, W), np.uint8) if want_u8 else None
        self.check(self.lib.roam_polar_to_cart_record_u8(self.h, _ptr(rec), rows, stride, payload_off, clip, _ptr(f), _ptr(u)))
        return f, u

    def warp_polar_f32(self, src, dsize_wh, center, max_radius, log=False, inverse=False):
        """cv2.warpPolar(src, dsize_wh, center, max_radius, INTER_LINEAR | WARP_FILL_OUTLIERS [| WARP_POLAR_LOG] [| WARP_INVERSE_MAP])
        on float32 (roam_warp_polar_f32).  src: (rows, cols) or a batch (n, rows, cols) of one geometry; dsize_wh = (dw, dh) already
        resolved (no OpenCV defaults here).  A 2-D float32 view with unit column stride is read in place with its row stride; any
        other input is made float32-contiguous first.  -> (dh, dw) or (n, dh, dw) float32"""
        a = np.asarray(src)
        if a.ndim not in (2, 3):
            raise ValueError(f"warp_polar_f32: a 2-D image or a 3-D batch, not {a.ndim}-D")
        if not (a.ndim == 2 and a.dtype == np.float32 and a.strides[1] == 4 and a.strides[0] % 4 == 0 and a.strides[0] >= 4 * a.shape[1]):
            a = np.ascontiguousarray(a, np.float32)
        batch = a.ndim == 3
        a3 = a if batch else a[None]
        n, rows, cols = a3.shape
        row_stride = a3.strides[1] // 4 if rows > 1 else cols
        image_stride = a3.strides[0] // 4 if n > 1 else rows * row_stride
        dw, dh = int(dsize_wh[0]), int(dsize_wh[1])
        out = np.empty((n, max(dh, 0), max(dw, 0)), np.float32)
        flags = (WARP_POLAR_LOG if log else 0) | (WARP_POLAR_INVERSE if inverse else 0)
        self.check(self.lib.roam_warp_polar_f32(self.h, _ptr(a3), n, rows, cols, row_stride, image_stride, _ptr(out), dw, dh,
                                                float(center[0]), float(center[1]), float(max_radius), flags))
        return out if batch else out[0]

    def warp_affine_f32(self, src, M, dsize_wh, inverse_map=False):
        """cv2.warpAffine(src, M, dsize_wh, INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT 0) on float32 (roam_warp_affine_f32,
        warpaffine.hip).  src: (rows, cols) or a batch (n, rows, cols) of one shape; M: (2, 3), or (n, 2, 3) - one matrix per image
        of the batch, all in one launch; dsize_wh = (dw, dh).  A 2-D float32 view with unit column stride is read in place with its
        row stride; any other input is made float32-contiguous first.  -> (dh, dw) or (n, dh, dw) float32.
        OpenCV adds the fixed-point terms of a source coordinate (1/1024 px each) in int32, so the map must keep every source
        coordinate below 2^20 px in magnitude: checked at the four corners of the output, with the other argument errors, by
        warp_affine_args (ValueError before any device call)."""
        a, m, dw, dh = warp_affine_args(src, M, dsize_wh, inverse_map)
        if not (a.ndim == 2 and a.dtype == np.float32 and a.strides[1] == 4 and a.strides[0] % 4 == 0 and a.strides[0] >= 4 * a.shape[1]):
            a = np.ascontiguousarray(a, np.float32)
        batch = a.ndim == 3
        a3 = a if batch else a[None]
        n, rows, cols = a3.shape
        row_stride = a3.strides[1] // 4 if rows > 1 else cols
        image_stride = a3.strides[0] // 4 if n > 1 else rows * row_stride
        out = np.empty((n, dh, dw), np.float32)
        self.check(self.lib.roam_warp_affine_f32(self.h, _ptr(a3), n, rows, cols, row_stride, image_stride, _ptr(m), len(m), _ptr(out),
                                                 dw, dh, WARP_AFFINE_INVERSE_MAP if inverse_map else 0))
        return out if batch else out[0]

    def time_warp_affine(self, n, rows, cols, M, reps=20):
        """milliseconds per launch of warp_affine_kernel on n resident rows x cols images warped by M into the same size, by HIP
        events after two warm runs (roam_time_warp_affine)"""
        m = np.ascontiguousarray(M, np.float64).reshape(6)
        ms = C.c_float(0)
        self.check(self.lib.roam_time_warp_affine(self.h, int(n), int(rows), int(cols), _ptr(m), int(reps), C.byref(ms)))
        return float(ms.value)

    def pyr_down_u8(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.empty(((h + 1) // 2, (w + 1) // 2), np.uint8)
        self.check(self.lib.roam_pyr_down_u8(self.h, _ptr(img), w, h, _ptr(out)))
        return out

    def pyr_down2_u8(self, buf, w, h, lanes, lane_stride, offs):
        """levels 2 and 3 of `lanes` pyramids from their w x h level 1, in place in `buf` (u8, the whole pyramid storage: level l of lane
        b at b * lane_stride + offs[l - 1]), by the two-level branch of the pyramid builder -> "rows" or "wave", the kernel it took"""
        assert buf.dtype == np.uint8 and buf.flags.c_contiguous and buf.ndim == 1
        k = C.c_int32(0)
        self.check(self.lib.roam_pyr_down2_u8(self.h, _ptr(buf), buf.size, int(w), int(h), int(lanes), int(lane_stride),
                                              int(offs[0]), int(offs[1]), int(offs[2]), C.byref(k)))
        return {1: "rows", 2: "wave"}[k.value]

    def klt_track(self, prev_img, next_img, pts, init_pts=None):
        """cv2.calcOpticalFlowPyrLK with the reference's LK_PARAMS -> (nextPts (K, 2) f32, status (K, 1) u8, err (K, 1) f32).  init_pts
        (K, 2): OPTFLOW_USE_INITIAL_FLOW, where the search for each feature starts (roam_klt_track_*_flow); None: at the feature.
        ValueError before any device call for what klt_flow_args refuses."""
        pts, init_pts = klt_flow_args(pts, init_pts)
        K = pts.shape[0]
        nxt = np.zeros((K, 2), np.float32)
        st = np.zeros((K,), np.uint8)
        err = np.zeros((K,), np.float32)
        h, w = prev_img.shape
        assert next_img.shape == prev_img.shape
        if prev_img.dtype == np.uint8:
            a, b = np.ascontiguousarray(prev_img), np.ascontiguousarray(next_img, np.uint8)
            fn, fn_flow = self.lib.roam_klt_track_u8, self.lib.roam_klt_track_u8_flow
        else:
            a, b = np.ascontiguousarray(prev_img, np.float32), np.ascontiguousarray(next_img, np.float32)
            fn, fn_flow = self.lib.roam_klt_track_f32, self.lib.roam_klt_track_f32_flow
        if init_pts is None:
            self.check(fn(self.h, _ptr(a), _ptr(b), w, h, _ptr(pts), K, _ptr(nxt), _ptr(st), _ptr(err)))
        else:
            self.check(fn_flow(self.h, _ptr(a), _ptr(b), w, h, _ptr(pts), _ptr(init_pts), K, _ptr(nxt), _ptr(st), _ptr(err)))
        return nxt, st.reshape(-1, 1), err.reshape(-1, 1)

    def reject_outliers(self, prev, new, thr_px, node_limit=0, want_adj=False):
        prev = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
        new = np.ascontiguousarray(new, np.float32).reshape(-1, 2)
        K = prev.shape[0]
        mask = np.zeros(K, np.uint8)
        n_in, flags = C.c_int32(0), C.c_int32(0)
        adj = np.zeros((K, max(1, (K + 63) // 64)), np.uint64) if want_adj else None
        self.check(self.lib.roam_reject_outliers(self.h, _ptr(prev), _ptr(new), K, float(thr_px), int(node_limit),
                                                 _ptr(mask), C.byref(n_in), C.byref(flags), _ptr(adj)))
        return mask.astype(bool), n_in.value, flags.value, adj

    def time_reject_outliers(self, prev, new, thr_px, copies=4096, reps=3, node_limit=0):
        """(graph ms, clique ms, inliers, proven) per launch of `copies` replicas of one correspondence set"""
        p = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
        n = np.ascontiguousarray(new, np.float32).reshape(-1, 2)
        g, q, ni, pr = C.c_float(0), C.c_float(0), C.c_int32(0), C.c_int32(0)
        self.check(self.lib.roam_time_reject_outliers(self.h, _ptr(p), _ptr(n), p.shape[0], int(copies), float(thr_px), int(node_limit), int(reps),
                                                      C.byref(g), C.byref(q), C.byref(ni), C.byref(pr)))
        return float(g.value), float(q.value), ni.value, bool(pr.value)

    def kabsch2d(self, src, tgt):
        s = np.ascontiguousarray(src, np.float64).reshape(-1, 2)
        t = np.ascontiguousarray(tgt, np.float64).reshape(-1, 2)
        R = np.empty((2, 2), np.float64)
        h = np.empty((2, 1), np.float64)
        self.check(self.lib.roam_kabsch2d(self.h, _ptr(s), _ptr(t), s.shape[0], _ptr(R), _ptr(h)))
        return R, h

    def mds_solve(self, T_wj0, p_w, p_jt, T_init, sigma5, period=0.25, want_debug=False):
        T0 = np.ascontiguousarray(T_wj0, np.float64)
        Ti = np.ascontiguousarray(T_init, np.float64)
        pw = np.ascontiguousarray(p_w[:, :2], np.float64)
        pj = np.ascontiguousarray(p_jt[:, :2], np.float64)
        sg = np.ascontiguousarray(sigma5, np.float64)
        N = pw.shape[0]
        out = np.empty(6)
        nfev, info = C.c_int32(0), C.c_int32(0)
        x0 = np.empty(6) if want_debug else None
        r0 = np.empty(2 * N + 3) if want_debug else None
        self.check(self.lib.roam_mds_solve(self.h, _ptr(T0), _ptr(pw), _ptr(pj), N, _ptr(Ti), _ptr(sg), float(period),
                                           _ptr(out), C.byref(nfev), C.byref(info), _ptr(x0), _ptr(r0)))
        return out, nfev.value, info.value, x0, r0

    def mds_undistort(self, v, pts, period=0.25):
        v = np.ascontiguousarray(v, np.float64)
        p = np.ascontiguousarray(pts[:, :2], np.float64)
        N = p.shape[0]
        xy = np.empty((N, 2))
        dT = np.empty(N)
        self.check(self.lib.roam_mds_undistort(self.h, _ptr(v), _ptr(p), N, float(period), _ptr(xy), _ptr(dT)))
        return xy, dT

    def ssc(self, kp, num_ret, tol, cols, rows):
        kp = np.ascontiguousarray(kp, np.float64)
        B = kp.shape[0]
        sel = np.empty(max(B, 1), np.int32)
        n = C.c_int32(0)
        self.check(self.lib.roam_ssc(self.h, _ptr(kp), B, int(num_ret), float(tol), int(cols), int(rows), _ptr(sel), C.byref(n)))
        return sel[:n.value]

    def fmt_rotation(self, src_polar, tgt_polar, clip_px=1012, downsample=10):
        """FMT.getRotationUsingFMT -> (angle rad, scale, response)"""
        a = np.ascontiguousarray(src_polar, np.float32)
        b = np.ascontiguousarray(tgt_polar, np.float32)
        assert a.shape == b.shape, "Images need to have the same shape!"
        ang, sc, rs = C.c_double(0), C.c_double(0), C.c_double(0)
        self.check(self.lib.roam_fmt_rotation(self.h, _ptr(a), _ptr(b), a.shape[0], a.shape[1], int(clip_px), int(downsample),
                                              C.byref(ang), C.byref(sc), C.byref(rs)))
        return ang.value, sc.value, rs.value

    def fmt_rotation_batch(self, src, tgt, clip_px=1012, downsample=10, want_logpolar=False):
        """FMT.getRotationUsingFMT for a batch of pairs in one device pass (roam_fmt_rotation_batch_f32): two 2-D polar images or two
        3-D batches of one shape -> (n, 3) float64 rows (angle rad, scale, response); want_logpolar: also the log-polar images before
        the window, (2 n, round(pi R), R) float32, all sources first, then all targets.  float32 views with unit column stride are
        read in place, anything else is made float32-contiguous.  Arguments are checked by fmt_rotation_batch_args before any device
        call."""
        a, b, clip, R = fmt_rotation_batch_args(src, tgt, clip_px, downsample)
        a3, b3, n, rows, cols, row_stride, image_stride = _batch_operands(a, b)
        out = np.empty((n, 3), np.float64)
        lp = np.empty((2 * n, int(np.rint(R * np.pi)), R), np.float32) if want_logpolar else None
        self.check(self.lib.roam_fmt_rotation_batch_f32(self.h, _ptr(a3), _ptr(b3), n, rows, cols, row_stride, image_stride, int(clip_px),
                                                        int(downsample), _ptr(out), _ptr(lp)))
        return (out, lp) if want_logpolar else out

    def fmt_register_batch(self, src, tgt, clip_px=1012, downsample=10, cart_downsample=20, want_images=False):
        """Fourier-Mellin registration of a batch of pairs in one device pass (roam_fmt_register_batch_f32): two 2-D polar images or
        two 3-D batches of one shape -> (n, 6) float64 rows (angle rad, scale, rotation response, dx, dy, translation response);
        columns 0-2 are fmt_rotation_batch's, (dx, dy) = phaseCorrelate(rotateImg(srcCart, degrees(angle)), tgtCart) in pixels of the
        Cartesian image at cart_downsample (metres: px * RANGE_RESOLUTION_M * cart_downsample).  want_images: also the Cartesian images
        before the window, (2 n, 2 Rc, 2 Rc) float32, Rc = cols // cart_downsample: the turned sources first, then the targets.
        float32 views with unit column stride are read in place, anything else is made float32-contiguous.  Arguments are checked by
        fmt_register_batch_args before any device call."""
        a, b, clip, R, Rc = fmt_register_batch_args(src, tgt, clip_px, downsample, cart_downsample)
        a3, b3, n, rows, cols, row_stride, image_stride = _batch_operands(a, b)
        out = np.empty((n, 6), np.float64)
        imgs = np.empty((2 * n, 2 * Rc, 2 * Rc), np.float32) if want_images else None
        self.check(self.lib.roam_fmt_register_batch_f32(self.h, _ptr(a3), _ptr(b3), n, rows, cols, row_stride, image_stride, int(clip_px),
                                                        int(downsample), int(cart_downsample), _ptr(out), _ptr(imgs)))
        return (out, imgs) if want_images else out

    def pose_graph_optimize(self, graphs, max_iterations=20, max_trials=10, lambda_init=0.0):
        """PoseGraphLib.PoseGraphOptimization.optimize for a batch of SE(2) pose graphs in one device pass
        (roam_pose_graph_optimize: g2o's EdgeSE2 and Levenberg-Marquardt, one workgroup per graph, no host round trip inside a
        solve).  graphs: a list of (poses (V, 3), fixed (V,), edge_ij (E, 2), meas (E, 3), info (E, 3, 3) or (3, 3), huber (E,) or
        None) -> (list of optimised poses (V, 3), stats: POSE_GRAPH_STATS rows).  The inputs are not modified.  A graph's result does
        not depend on the batch.  Arguments are checked by pose_graph_args before any library call; the cost of a graph is its
        envelope (pose_graph_plan)."""
        vertex_off, poses, fixed, edge_off, ij, meas, info, huber, opts = pose_graph_args(graphs, max_iterations, max_trials, lambda_init)
        n = len(vertex_off) - 1
        stats = np.zeros(n, POSE_GRAPH_STATS)
        self.check(self.lib.roam_pose_graph_optimize(self.h, n, _ptr(vertex_off), _ptr(poses), _ptr(fixed), _ptr(edge_off), _ptr(ij),
                                                     _ptr(meas), _ptr(info), _ptr(huber), C.byref(opts), _ptr(stats)))
        return [poses[vertex_off[g]:vertex_off[g + 1]].copy() for g in range(n)], stats

    def icp2d_batch(self, pairs, init=None, opts=None):
        """Trimmed point-to-point ICP in the plane for a batch of cloud pairs in one device pass (roam_icp2d_batch: one workgroup per
        pair, exhaustive float32 nearest-neighbour search, float64 closed-form update, the gate shrinking from gate_start to gate_end).
        pairs: a list of (src (n, 2), dst (m, 2)); init: (3,) or (len(pairs), 3) rows (theta, tx, ty); opts: None, a dict over
        ICP_DEFAULTS or an IcpOpts -> (poses (len(pairs), 3) rows (theta, tx, ty) with dst ~ R(theta) src + t, stats: ICP_STATS rows).
        A pair's result does not depend on the batch.  Arguments are checked by icp2d_args before any library call."""
        src_off, src, dst_off, dst, x0, o = icp2d_args(pairs, init, opts)
        n = len(src_off) - 1
        poses, stats = np.empty((n, 3), np.float64), np.zeros(n, ICP_STATS)
        self.check(self.lib.roam_icp2d_batch(self.h, n, _ptr(src_off), _ptr(src), _ptr(dst_off), _ptr(dst), _ptr(x0), C.byref(o), _ptr(poses),
                                             _ptr(stats)))
        return poses, stats

    def time_icp2d_batch(self, pairs, init=None, opts=None, reps=5):
        """milliseconds per launch of the ICP kernel on these pairs (roam_time_icp2d_batch: events, two warm launches first)"""
        src_off, src, dst_off, dst, x0, o = icp2d_args(pairs, init, opts)
        ms = C.c_float()
        self.check(self.lib.roam_time_icp2d_batch(self.h, len(src_off) - 1, _ptr(src_off), _ptr(src), _ptr(dst_off), _ptr(dst), _ptr(x0),
                                                  C.byref(o), int(reps), C.byref(ms)))
        return ms.value

    def scan_context_offsets(self, polar, offsets_m, range_resolution_m, sectors=60, rings=20, clip_px=None, floor=0.0):
        """scan_context with the origin-shifted variants (roam_scan_context_offsets_f32) -> (n, 1 + n_offsets, sectors, rings) float32:
        variant 0 the plain descriptor, variant a the scan as seen from offsets_m[a - 1] (metres, x = r cos phi, y = r sin phi).
        ValueError before any library call"""
        a3, n, rows, cols, row_stride, image_stride, _ = scan_context_images(polar, clip_px, sectors, rings)
        floor = scan_context_floor(floor)
        off, res = loop_offsets_args(offsets_m, range_resolution_m)
        if n * len(off) * sectors * rings * 4 > LOOP_DB_BYTES:
            raise ValueError(f"scan context offsets: {n} images x {len(off)} offsets are beyond {LOOP_DB_BYTES} bytes of descriptors")
        out = np.empty((n, 1 + len(off), sectors, rings), np.float32)
        self.check(self.lib.roam_scan_context_offsets_f32(self.h, _ptr(a3), n, rows, cols, row_stride, image_stride, int(clip_px or 0), int(sectors),
                                                          int(rings), floor, len(off), _ptr(off), res, _ptr(out)))
        return out

    def scan_context(self, polar, sectors=60, rings=20, clip_px=None, floor=0.0):
        """the scan-context descriptors of a 2-D float32 polar image or a 3-D batch (roam_scan_context_f32) -> (n, sectors, rings)
        float32: the area mean of max(v - floor, 0) over integer bins (scan_context_plan).  ValueError before any library call"""
        a3, n, rows, cols, row_stride, image_stride, _ = scan_context_images(polar, clip_px, sectors, rings)
        floor = scan_context_floor(floor)
        out = np.empty((n, sectors, rings), np.float32)
        self.check(self.lib.roam_scan_context_f32(self.h, _ptr(a3), n, rows, cols, row_stride, image_stride, int(clip_px or 0), int(sectors),
                                                  int(rings), floor, _ptr(out)))
        return out

    def phase_correlate(self, src, tgt, hanning=True):
        """FMT.getTranslationUsingPhaseCorrelation: cv2.phaseCorrelate(src, tgt[, cv2.createHanningWindow((cols, rows), CV_32F)])
        (roam_phase_correlate_f32).  Two 2-D images -> ((dx, dy), response); two 3-D batches of one shape -> (dxdy (n, 2),
        response (n,)).  float32 views with unit column stride are read in place, anything else is made float32-contiguous."""
        a, b = phase_correlate_args(src, tgt)
        batch = a.ndim == 3
        a3, b3, n, rows, cols, row_stride, image_stride = _batch_operands(a, b)
        dxdy = np.empty((n, 2), np.float64)
        resp = np.empty(n, np.float64)
        self.check(self.lib.roam_phase_correlate_f32(self.h, _ptr(a3), _ptr(b3), n, rows, cols, row_stride, image_stride,
                                                     1 if hanning else 0, _ptr(dxdy), _ptr(resp)))
        if batch:
            return dxdy, resp
        return (float(dxdy[0, 0]), float(dxdy[0, 1])), float(resp[0])

    def debug_fft2(self, plane, inverse=False):
        """test entry: the 2-D FFT of csrc/fft.hip alone on one complex (or real) float64 plane -> complex128; inverse: unscaled"""
        z = np.asarray(plane)
        re = np.ascontiguousarray(z.real, np.float64)
        im = np.ascontiguousarray(z.imag, np.float64) if np.iscomplexobj(z) else None
        rows, cols = re.shape
        ro, io = np.empty_like(re), np.empty_like(re)
        self.check(self.lib.roam_debug_fft2_f64(self.h, _ptr(re), _ptr(im), rows, cols, 1 if inverse else 0, _ptr(ro), _ptr(io)))
        return ro + 1j * io

    def debug_ssc_batch(self, kp, count, num_ret, tol, cols, rows, n_active=None, first=0):
        """test entry: the engine's batched SSC kernel alone (roam_debug_ssc_batch).  kp (P, kp_cap, 3) float64, count (P,) -> (sel
        (P, kp_cap) int32, n_sel (P,) int32), both prefilled with -1: a problem at or beyond n_active - first keeps it"""
        kp = np.ascontiguousarray(kp, np.float64)
        P, kp_cap, three = kp.shape
        assert three == 3
        count = np.ascontiguousarray(count, np.int32)
        assert count.shape == (P,)
        sel = np.zeros((P, kp_cap), np.int32)
        n_sel = np.zeros(P, np.int32)
        self.check(self.lib.roam_debug_ssc_batch(self.h, _ptr(kp), _ptr(count), P, kp_cap, P if n_active is None else int(n_active), int(first),
                                                 int(num_ret), float(tol), int(cols), int(rows), _ptr(sel), _ptr(n_sel)))
        return sel, n_sel

    def debug_mds_solve_batch(self, T_wj0, p_w, p_jt, count, nmax, T_init, sigma5, period=0.25, big=False, repeat=1, want_list=False):
        """test entry: the motion-distortion solve as the engine launches it (roam_debug_mds_solve_batch).  T_wj0, T_init (B, 3, 3),
        p_w, p_jt (B, nstride, 2), count (B,), nmax <= nstride; big: with the list that hands the large problems to the workgroup
        kernel; repeat consecutive solves -> (out6 (repeat, B, 6), nfev (repeat, B), info (repeat, B)); want_list: and the list's two
        slots (2, 1 + B) [n, ids ...] as the last solve left them"""
        T0 = np.ascontiguousarray(T_wj0, np.float64)
        Ti = np.ascontiguousarray(T_init, np.float64)
        pw = np.ascontiguousarray(p_w, np.float64)
        pj = np.ascontiguousarray(p_jt, np.float64)
        cnt = np.ascontiguousarray(count, np.int32)
        sg = np.ascontiguousarray(sigma5, np.float64)
        B, nstride, two = pw.shape
        assert two == 2 and pj.shape == pw.shape and T0.shape == Ti.shape == (B, 3, 3) and cnt.shape == (B,) and sg.shape == (5,)
        out = np.zeros((repeat, B, 6))
        nfev = np.zeros((repeat, B), np.int32)
        info = np.zeros((repeat, B), np.int32)
        lists = np.zeros((2, 1 + B), np.int32) if want_list else None
        self.check(self.lib.roam_debug_mds_solve_batch(self.h, _ptr(T0), _ptr(pw), _ptr(pj), _ptr(cnt), B, nstride, int(nmax), _ptr(Ti),
                                                       _ptr(sg), float(period), 1 if big else 0, int(repeat), _ptr(out), _ptr(nfev),
                                                       _ptr(info), _ptr(lists)))
        return (out, nfev, info, lists) if want_list else (out, nfev, info)

    def debug_lm_lmpar(self, R, ipvt, qtb, delta, par_in, form):
        """test entry: lmpar alone (roam_debug_lm_lmpar), diag = 1.  form 0: the workgroup kernel's copy -> (par (1,), x (1, 6), sdiag
        (1, 6)); form 1: the one-wavefront kernel's, as stored by lanes 0 and 63 -> (par (2,), x (2, 6), sdiag (2, 6))"""
        R = np.ascontiguousarray(R, np.float64)
        ip = np.ascontiguousarray(ipvt, np.int32)
        q = np.ascontiguousarray(qtb, np.float64)
        assert R.shape == (6, 6) and ip.shape == (6,) and q.shape == (6,)
        k = 2 if form else 1
        par, x, sd = np.zeros(k), np.zeros((k, 6)), np.zeros((k, 6))
        self.check(self.lib.roam_debug_lm_lmpar(self.h, 6, _ptr(R), _ptr(ip), _ptr(q), float(delta), float(par_in), int(form), _ptr(par),
                                                _ptr(x), _ptr(sd)))
        return par, x, sd

    def time_fft2(self, rows, cols, what, reps=20):
        """milliseconds per repetition of `what` (TIME_*) at rows x cols, by HIP events after two warm runs"""
        ms = C.c_float(0)
        self.check(self.lib.roam_time_fft2(self.h, int(rows), int(cols), int(what), int(reps), C.byref(ms)))
        return float(ms.value)

    def doh_maxima(self, img, sigmas, threshold, cap=1 << 18):
        """-> (rcs (n,3) int32 [row, col, sigma_index] in C order, values (n,) f64)"""
        img = np.ascontiguousarray(img, np.float32)
        h, w = img.shape
        sig = np.ascontiguousarray(sigmas, np.float64)
        rcs = np.empty((cap, 3), np.int32)
        val = np.empty(cap, np.float64)
        n = C.c_int32(0)
        self.check(self.lib.roam_doh_maxima(self.h, _ptr(img), w, h, _ptr(sig), len(sig), float(threshold), _ptr(rcs),
                                            _ptr(val), cap, C.byref(n)))
        return rcs[:n.value], val[:n.value]

    def log_maxima(self, img, sigma_list, threshold, want_layers=False, cap=1 << 17):
        """Laplacian-of-Gaussian scale space of blob_log and its 3x3x3 maxima.  img: f32 (widened exactly on the device) or
        f64; anything else is converted to f64 first.  sigma_list: scalar sigmas.  -> (rcs (n,3) int32 [row, col, sigma_index]
        in C order, values (n,) f64[, layers (num_sigma, h, w) f64 = -gaussian_laplace(img, s) * s**2])"""
        from .gaussian import laplace_kernels
        img = np.asarray(img)
        img = np.ascontiguousarray(img, np.float32 if img.dtype == np.float32 else np.float64)
        h, w = img.shape
        sig = np.asarray(sigma_list, np.float64).reshape(-1)
        ks = [laplace_kernels(s) for s in sig]
        radius = np.array([k[0] for k in ks], np.int32)
        kernels = np.ascontiguousarray(np.concatenate([np.concatenate([k0, k2]) for _, k0, k2 in ks]), np.float64)
        scale = np.array([s * s for s in sig], np.float64)
        layers = np.empty((len(sig), h, w), np.float64) if want_layers else None
        for attempt in range(2):
            rcs = np.empty((max(cap, 1), 3), np.int32)
            val = np.empty(max(cap, 1), np.float64)
            n = C.c_int32(0)
            rc = self.lib.roam_log_maxima(self.h, _ptr(img), img.itemsize, w, h, len(sig), _ptr(radius), _ptr(kernels), _ptr(scale),
                                          float(threshold), _ptr(rcs), _ptr(val), cap, C.byref(n), _ptr(layers))
            if rc == ROAM_E_CAPACITY and attempt == 0:
                cap = n.value
                continue
            self.check(rc)
            break
        out = (rcs[:n.value], val[:n.value])
        return out + (layers,) if want_layers else out


_default = {}
_lock = threading.Lock()


class LoopDb:
    """A database of scan-context descriptors in HBM (roam_loop_db): add, then query.  Bound to the context it was made on (None: the
    default context, asked for after the arguments have passed).  After keep_clouds every described scan also stores its polar peak
    cloud in metres, and verify / query_verify run the ICP of Context.icp2d_batch from that store."""

    def __init__(self, ctx, capacity: int, sectors: int = 60, rings: int = 20):
        for name, v, lo, hi in (("capacity", capacity, 1, 2 ** 31 - 1), ("sectors", sectors, 2, SCAN_CONTEXT_MAX_SECTORS),
                                ("rings", rings, 1, SCAN_CONTEXT_MAX_RINGS)):
            if not isinstance(v, numbers.Integral) or isinstance(v, bool) or not lo <= v <= hi:
                raise ValueError(f"loop db: {name} an integer in [{lo}, {hi}], not {v!r}")
        per = sectors * (4 * rings + 8 * ((rings + 3) & ~3) + 4)
        if capacity > LOOP_DB_BYTES // per:
            raise ValueError(f"loop db: capacity at most {LOOP_DB_BYTES // per} ({per} bytes per entry, {LOOP_DB_BYTES} in all), not {capacity}")
        ctx = ctx or default_context()
        self.ctx, self.capacity, self.sectors, self.rings = ctx, int(capacity), int(sectors), int(rings)
        h = _vp()
        ctx.check(ctx.lib.roam_loop_db_create(ctx.h, self.capacity, self.sectors, self.rings, C.byref(h)))
        self.h = h
        self.cloud_rows = self.max_points = None             # set by keep_clouds
        self.offsets_m = None                                # set by keep_offsets: (n_offsets, 2) float64 metres

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.roam_loop_db_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = C.c_int32(0)
        self.ctx.check(self.ctx.lib.roam_loop_db_count(self.h, C.byref(n)))
        return n.value

    def add_f32(self, polar, clip_px=None, floor=0.0):
        """describe a 2-D float32 polar image or a 3-D batch on the device and append -> the index of the first new entry"""
        a3, n, rows, cols, row_stride, image_stride, _ = scan_context_images(polar, clip_px, self.sectors, self.rings)
        floor = scan_context_floor(floor)
        first = C.c_int32(-1)
        self.ctx.check(self.ctx.lib.roam_loop_db_add_f32(self.ctx.h, self.h, _ptr(a3), n, rows, cols, row_stride, image_stride,
                                                         int(clip_px or 0), floor, C.byref(first)))
        return first.value

    def add_desc(self, desc):
        """append ready-made descriptors, (S, R) or (n, S, R) -> the index of the first new entry"""
        d = np.ascontiguousarray(desc, np.float32)
        d = d[None] if d.ndim == 2 else d
        if d.ndim != 3 or d.shape[0] < 1 or d.shape[1:] != (self.sectors, self.rings):
            raise ValueError(f"loop db: descriptors (n, {self.sectors}, {self.rings}), not {d.shape}")
        if not np.isfinite(d).all():
            raise ValueError("loop db: a descriptor value that is not finite")
        first = C.c_int32(-1)
        self.ctx.check(self.ctx.lib.roam_loop_db_add_desc(self.ctx.h, self.h, _ptr(d), len(d), C.byref(first)))
        return first.value

    def get(self, first=0, n=None):
        count = len(self)
        n = count - first if n is None else n
        if first < 0 or n < 1 or first + n > count:
            raise ValueError(f"loop db: entries [{first}, {first} + {n}) outside the {count} stored")
        out = np.empty((n, self.sectors, self.rings), np.float32)
        self.ctx.check(self.ctx.lib.roam_loop_db_get(self.ctx.h, self.h, int(first), int(n), _ptr(out)))
        return out

    def query(self, indices, max_index, k=8, max_distance=np.inf, want_full=False):
        """roam_loop_db_query: for each query entry the k candidates among the entries below its max_index with distance <=
        max_distance -> (index (m, k) int32, distance (m, k) float64, shift (m, k) int32); unused slots -1, +inf, 0.  want_full: also
        the (m, count) distance and shift to every entry"""
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        ci, cd, cs = np.empty((len(q), k), np.int32), np.empty((len(q), k), np.float64), np.empty((len(q), k), np.int32)
        df = np.empty((len(q), len(self)), np.float64) if want_full else None
        sf = np.empty((len(q), len(self)), np.int32) if want_full else None
        self.ctx.check(self.ctx.lib.roam_loop_db_query(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance), _ptr(ci),
                                                       _ptr(cd), _ptr(cs), _ptr(df), _ptr(sf)))
        return (ci, cd, cs, df, sf) if want_full else (ci, cd, cs)

    # ---- origin-shifted variants
    def keep_offsets(self, offsets_m, range_resolution_m=0.0432):
        """roam_loop_db_keep_offsets: once, on an empty database - from here on every described scan also stores its descriptor as
        seen from each of the offsets (metres), and query_offsets / query_verify take the minimum over these variants"""
        off, res = loop_offsets_args(offsets_m, range_resolution_m, self.capacity, self.sectors, self.rings)
        if self.offsets_m is not None:
            raise ValueError("loop db: keeps offsets already")
        if len(self):
            raise ValueError(f"loop db: keep_offsets on an empty database, not one of {len(self)} entries")
        self.ctx.check(self.ctx.lib.roam_loop_db_keep_offsets(self.ctx.h, self.h, len(off), _ptr(off), res))
        self.offsets_m = off

    def _needs_offsets(self):
        if self.offsets_m is None:
            raise ValueError("loop db: keeps no offsets (keep_offsets)")

    def _entry(self, index):
        if not isinstance(index, numbers.Integral) or isinstance(index, bool) or not 0 <= index < len(self):
            raise ValueError(f"loop db: index in [0, {len(self)}), not {index!r}")
        return int(index)

    def set_variants(self, index, desc):
        """replace the variants 1 .. n_offsets of the stored entry `index` by desc (n_offsets, S, R)"""
        self._needs_offsets()
        d = np.ascontiguousarray(desc, np.float32)
        if d.shape != (len(self.offsets_m), self.sectors, self.rings):
            raise ValueError(f"loop db: variants ({len(self.offsets_m)}, {self.sectors}, {self.rings}), not {d.shape}")
        if not np.isfinite(d).all():
            raise ValueError("loop db: a descriptor value that is not finite")
        self.ctx.check(self.ctx.lib.roam_loop_db_set_variants(self.ctx.h, self.h, self._entry(index), _ptr(d)))

    def get_variants(self, index):
        """-> (desc (n_offsets, S, R) float32, valid (n_offsets, S) int32) of the stored entry `index`"""
        self._needs_offsets()
        d = np.empty((len(self.offsets_m), self.sectors, self.rings), np.float32)
        v = np.empty((len(self.offsets_m), self.sectors), np.int32)
        self.ctx.check(self.ctx.lib.roam_loop_db_get_variants(self.ctx.h, self.h, self._entry(index), _ptr(d), _ptr(v)))
        return d, v

    def query_offsets(self, indices, max_index, k=8, max_distance=np.inf, want_full=False):
        """roam_loop_db_query_offsets: query over the variants of the query entries -> query's arrays plus the winning variant
        (m, k) int32 (0: the plain descriptor, a: offsets_m[a - 1]); want_full: also (m, count) distance, shift and variant"""
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        ci, cd, cs = np.empty((len(q), k), np.int32), np.empty((len(q), k), np.float64), np.empty((len(q), k), np.int32)
        cv = np.empty((len(q), k), np.int32)
        df = np.empty((len(q), len(self)), np.float64) if want_full else None
        sf = np.empty((len(q), len(self)), np.int32) if want_full else None
        vf = np.empty((len(q), len(self)), np.int32) if want_full else None
        self.ctx.check(self.ctx.lib.roam_loop_db_query_offsets(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance), _ptr(ci),
                                                               _ptr(cd), _ptr(cs), _ptr(cv), _ptr(df), _ptr(sf), _ptr(vf)))
        return (ci, cd, cs, cv, df, sf, vf) if want_full else (ci, cd, cs, cv)

    def variant_offsets(self, variant):
        """variant indices (...) -> their offsets in metres (..., 2); variant 0 (and a database without offsets) is (0, 0)"""
        table = np.zeros((1, 2)) if self.offsets_m is None else np.concatenate([np.zeros((1, 2)), self.offsets_m])
        return table[np.asarray(variant)]

    def query_verify_offsets(self, indices, max_index, k=8, max_distance=np.inf, opts=None):
        """roam_loop_db_query_verify_offsets: query_verify plus the winning variants (m, k) int32 before the poses"""
        self._needs_clouds()
        o = icp2d_opts(opts)
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        ci, cd, cs = np.empty((len(q), k), np.int32), np.empty((len(q), k), np.float64), np.empty((len(q), k), np.int32)
        cv = np.empty((len(q), k), np.int32)
        poses, stats = np.empty((len(q), k, 3), np.float64), np.zeros((len(q), k), ICP_STATS)
        self.ctx.check(self.ctx.lib.roam_loop_db_query_verify_offsets(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance),
                                                                      C.byref(o), _ptr(ci), _ptr(cd), _ptr(cs), _ptr(cv), _ptr(poses), _ptr(stats)))
        return ci, cd, cs, cv, poses, stats

    def time_query_offsets(self, indices, max_index, k=8, max_distance=np.inf, reps=20):
        """(plain distance kernel ms, variants' distance kernel and fold ms, selection kernel ms) per launch
        (roam_time_loop_db_query_offsets)"""
        self._needs_offsets()
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        self.ctx.check(self.ctx.lib.roam_time_loop_db_query_offsets(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance),
                                                                    int(reps), C.byref(a), C.byref(b), C.byref(c)))
        return float(a.value), float(b.value), float(c.value)

    # ---- peak clouds
    def keep_clouds(self, rows, max_points=ICP_MAX_POINTS, point_stride=1, range_resolution_m=0.0432):
        """roam_loop_db_keep_clouds: once, on an empty database - from here on every described scan (`rows` azimuths) stores its polar
        peaks in metres beside the descriptor: every step-th peak, step = max(point_stride, ceil(peaks / max_points))"""
        rows, mp, ps, res = loop_cloud_args(self.capacity, rows, max_points, point_stride, range_resolution_m)
        if self.cloud_rows is not None:
            raise ValueError("loop db: keeps clouds already")
        self.ctx.check(self.ctx.lib.roam_loop_db_keep_clouds(self.ctx.h, self.h, rows, mp, ps, res))
        self.cloud_rows, self.max_points = rows, mp

    def _needs_clouds(self):
        if self.cloud_rows is None:
            raise ValueError("loop db: keeps no clouds (keep_clouds)")

    def set_cloud(self, index, xy):
        """replace the cloud of the stored entry `index` by xy (n, 2) metres, n <= max_points"""
        self._needs_clouds()
        a = loop_cloud_points(xy, self.max_points)
        if not isinstance(index, numbers.Integral) or isinstance(index, bool) or not 0 <= index < len(self):
            raise ValueError(f"loop db: index in [0, {len(self)}), not {index!r}")
        self.ctx.check(self.ctx.lib.roam_loop_db_set_cloud(self.ctx.h, self.h, int(index), _ptr(a), len(a)))

    def cloud_counts(self):
        """-> (points stored (count,), peaks of the scan (count,)) int32 of every entry; no device call"""
        self._needs_clouds()
        n = len(self)
        a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.ctx.check(self.ctx.lib.roam_loop_db_cloud_counts(self.h, 0, n, _ptr(a), _ptr(b)))
        return a, b

    def get_cloud(self, index):
        """-> (xy (n, 2) float64 metres, the scan's full peak count)"""
        self._needs_clouds()
        if not isinstance(index, numbers.Integral) or isinstance(index, bool) or not 0 <= index < len(self):
            raise ValueError(f"loop db: index in [0, {len(self)}), not {index!r}")
        xy = np.empty((self.max_points, 2), np.float64)
        n, n_peaks = C.c_int32(0), C.c_int32(0)
        self.ctx.check(self.ctx.lib.roam_loop_db_get_cloud(self.ctx.h, self.h, int(index), _ptr(xy), self.max_points, C.byref(n), C.byref(n_peaks)))
        return xy[:n.value].copy(), n_peaks.value

    def verify(self, src_index, dst_index, init=None, opts=None):
        """roam_loop_db_verify: the ICP of Context.icp2d_batch on pairs of stored clouds, entry src_index[p] onto entry dst_index[p] from
        init -> (poses (n, 3), stats: ICP_STATS rows), bit for bit what icp2d_batch gives on the same clouds"""
        self._needs_clouds()
        o = icp2d_opts(opts)
        si, di, x0 = loop_verify_args(len(self), src_index, dst_index, init)
        poses, stats = np.empty((len(si), 3), np.float64), np.zeros(len(si), ICP_STATS)
        self.ctx.check(self.ctx.lib.roam_loop_db_verify(self.ctx.h, self.h, len(si), _ptr(si), _ptr(di), _ptr(x0), C.byref(o), _ptr(poses), _ptr(stats)))
        return poses, stats

    def time_verify(self, src_index, dst_index, init=None, opts=None, reps=5):
        """milliseconds per launch of the ICP kernel on these stored pairs (roam_time_loop_db_verify)"""
        self._needs_clouds()
        o = icp2d_opts(opts)
        si, di, x0 = loop_verify_args(len(self), src_index, dst_index, init)
        ms = C.c_float(0)
        self.ctx.check(self.ctx.lib.roam_time_loop_db_verify(self.ctx.h, self.h, len(si), _ptr(si), _ptr(di), _ptr(x0), C.byref(o), int(reps), C.byref(ms)))
        return float(ms.value)

    def query_verify(self, indices, max_index, k=8, max_distance=np.inf, opts=None):
        """roam_loop_db_query_verify: query, then every (query, slot) verified from the stored clouds with the seed (yaw of the shift,
        0, 0), one device pass and one read-back -> (index (m, k), distance (m, k), shift (m, k), poses (m, k, 3), stats (m, k)
        ICP_STATS); an unused slot is ICP_FEW_PAIRS at the seed (0, 0, 0)"""
        self._needs_clouds()
        o = icp2d_opts(opts)
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        ci, cd, cs = np.empty((len(q), k), np.int32), np.empty((len(q), k), np.float64), np.empty((len(q), k), np.int32)
        poses, stats = np.empty((len(q), k, 3), np.float64), np.zeros((len(q), k), ICP_STATS)
        self.ctx.check(self.ctx.lib.roam_loop_db_query_verify(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance), C.byref(o),
                                                              _ptr(ci), _ptr(cd), _ptr(cs), _ptr(poses), _ptr(stats)))
        return ci, cd, cs, poses, stats

    # ---- the global map
    def map_bounds(self, poses, use=None):
        """roam_loop_db_map_bounds: (bounds (4,) float64 = min x, max x, min y, max y of the used entries' points at these poses, their
        number); no point: (+inf, -inf, +inf, -inf), 0"""
        self._needs_clouds()
        p, u, _, _, _, _ = loop_map_args(len(self), poses, use)
        b, n = np.empty(4, np.float64), C.c_int64(0)
        self.ctx.check(self.ctx.lib.roam_loop_db_map_bounds(self.ctx.h, self.h, _ptr(p), _ptr(u), _ptr(b), C.byref(n)))
        return b, n.value

    def map_render(self, poses, res, extent, min_hits=1, min_views=1, use=None, grids=True, cap=None):
        """roam_loop_db_map_render on the extent (ox, oy, W, H) -> dict: hits, views (H, W) uint32 (None without grids), points (M, 2)
        float64, point_hits, point_views (M,) uint32, outside.  cap (None: as many as there can be - the cells, or the used entries'
        points if those are fewer): more map points than that raise RoamError ROAM_E_CAPACITY, its .required the count"""
        self._needs_clouds()
        p, u, res, extent, min_hits, min_views = loop_map_args(len(self), poses, use, res, extent, min_hits, min_views)
        if extent is None:
            raise ValueError("global map: extent (ox, oy, W, H), not None")
        ox, oy, W, H = extent
        if cap is None:
            n = self.cloud_counts()[0].astype(np.int64)
            cap = int(min(W * H, n.sum() if u is None else n[u != 0].sum()))
        if not isinstance(cap, numbers.Integral) or isinstance(cap, bool) or not 0 <= cap < 2 ** 31:
            raise ValueError(f"global map: cap an integer >= 0, not {cap!r}")
        hits, views = (np.empty((H, W), np.uint32), np.empty((H, W), np.uint32)) if grids else (None, None)
        pts, ph, pv = np.empty((cap, 2), np.float64), np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        m, outside = C.c_int32(0), C.c_int64(0)
        rc = self.ctx.lib.roam_loop_db_map_render(self.ctx.h, self.h, _ptr(p), _ptr(u), res, ox, oy, W, H, min_hits, min_views, _ptr(hits),
                                                  _ptr(views), _ptr(pts), _ptr(ph), _ptr(pv), int(cap), C.byref(m), C.byref(outside))
        if rc == ROAM_E_CAPACITY:
            err = RoamError(rc, self.ctx.lib.roam_last_error(self.ctx.h).decode(errors="replace"))
            err.required = m.value
            raise err
        self.ctx.check(rc)
        return dict(hits=hits, views=views, points=pts[:m.value].copy(), point_hits=ph[:m.value].copy(), point_views=pv[:m.value].copy(),
                    outside=outside.value)

    def time_map(self, poses, res, extent, min_hits=1, min_views=1, use=None, reps=5):
        """(clear ms, splat ms, compaction ms) per launch of this render's three parts (roam_time_loop_db_map)"""
        self._needs_clouds()
        p, u, res, extent, min_hits, min_views = loop_map_args(len(self), poses, use, res, extent, min_hits, min_views)
        if extent is None:
            raise ValueError("global map: extent (ox, oy, W, H), not None")
        ms = (C.c_float * 3)()
        self.ctx.check(self.ctx.lib.roam_time_loop_db_map(self.ctx.h, self.h, _ptr(p), _ptr(u), res, *extent, min_hits, min_views, int(reps), ms))
        return tuple(float(v) for v in ms)

    def time_query(self, indices, max_index, k=8, max_distance=np.inf, reps=20):
        """(distance kernel ms, selection kernel ms) per launch of this query, HIP events around reps launches (roam_time_loop_db_query)"""
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        d_ms, s_ms = C.c_float(0), C.c_float(0)
        self.ctx.check(self.ctx.lib.roam_time_loop_db_query(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance), int(reps),
                                                            C.byref(d_ms), C.byref(s_ms)))
        return float(d_ms.value), float(s_ms.value)


def default_context(device_id: int = None) -> Context:
    """Process-wide context per device (lazily created); device from ROAM_DEVICE / LOCAL_RANK."""
    if device_id is None:
        device_id = int(os.environ.get("ROAM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _lock:
        if device_id not in _default:
            _default[device_id] = Context(device_id)
        return _default[device_id]
