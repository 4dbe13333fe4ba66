"""What include/roam_abi.h declares, restated for ctypes and numpy: return codes, flags and limits, the structs, the signature of
every entry.  Nothing here loads or calls the library; tests/test_abi_mirror_cpu.py holds all of it against the header."""
import ctypes as C

import numpy as np

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
KLT_MAX_GUESS = float(1 << 20)          # ROAM_KLT_MAX_GUESS
PRIOR_MAX_LINEAR = 64.0                 # ROAM_PRIOR_MAX_LINEAR
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
# map matching: roam_abi.h ROAM_MATCH_MAX_RADIUS, _ANGLES, _SHIFT and _VOLUME (tests/test_map_match_cpu.py holds them against the header)
MAP_MATCH_MAX_RADIUS, MAP_MATCH_MAX_ANGLES, MAP_MATCH_MAX_SHIFT, MAP_MATCH_MAX_VOLUME = 8, 1025, 128, 1 << 26
MAP_MATCH_MAX_QUERIES = 65535           # queries of one roam_map_match_clouds / roam_loop_db_map_match call
# MapLocalizer.match's rows, one per query: what roam_map_match_clouds returns in pose_out and info_out, and what follows from it
MATCH_TABLE = np.dtype([("x", np.float64), ("y", np.float64), ("theta", np.float64), ("score", np.uint32), ("fraction", np.float64),
                        ("nPoints", np.int32), ("nInside", np.int32), ("i", np.int32), ("b", np.int32), ("a", np.int32), ("found", np.bool_)])


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
    "roam_cloud_motion_table": (C.c_int32, [C.c_int32, C.c_double, C.c_int32, _vp, _vp]),
    "roam_loop_db_add_f32_motion": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double,
                                                _vp, C.c_double, _P(C.c_int32)]),
    "roam_engine_loop_db_add_motion": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, C.c_double, _P(C.c_int32)]),
    "roam_engine_time_loop_cloud_motion": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_double, C.c_int32, _P(C.c_float), _P(C.c_float)]),
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
    "roam_map_field_table": (C.c_int32, [C.c_double, C.c_int32, _vp]),
    "roam_map_field_create": (C.c_int32, [_vp, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp,
                                          _P(_vp)]),
    "roam_map_field_read": (C.c_int32, [_vp, _vp, _vp]),
    "roam_map_field_destroy": (C.c_int32, [_vp, _vp]),
    "roam_map_match_angles": (C.c_int32, [C.c_int32, _vp, C.c_int32, C.c_double, _vp]),
    "roam_map_match_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "roam_map_match_clouds": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "roam_loop_db_map_match": (C.c_int32, [_vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "roam_time_map_match": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_double,
                                        C.c_int32, C.c_int32, C.c_int32, _vp]),
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
