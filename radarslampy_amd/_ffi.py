"""ctypes binding of libroam_hip.so (include/roam_abi.h).  No torch, no CPU fallback: if
the HIP library or a gfx950 device is missing every compute call raises RoamError.
This module is what touches the library: the loader, the host-only plan / table wrappers, Context and LoopDb.  The header's mirror
is _abi.py and the checks that call nothing are _args.py; every name of both is re-exported here, by name."""
import ctypes as C
import numbers
import os
import threading

import numpy as np

from ._abi import (ABI_SYMBOLS, COMM_ID_BYTES, FMT_MAX_COLS, FMT_MAX_R, FMT_MAX_ROWS, FMT_MIN_R, ICP_DEFAULTS, ICP_FEW_PAIRS,
                   ICP_ITERATION_LIMIT, ICP_MAX_COORD, ICP_MAX_ITERATIONS, ICP_MAX_PAIRS, ICP_MAX_POINTS, ICP_OK, ICP_STATS, KLT_MAX_GUESS,
                   LOOP_DB_BYTES, LOOP_MAX_K, LOOP_MAX_OFFSETS, MAP_MATCH_MAX_ANGLES, MAP_MATCH_MAX_QUERIES, MAP_MATCH_MAX_RADIUS,
                   MAP_MATCH_MAX_SHIFT, MAP_MATCH_MAX_VOLUME, MAP_MAX_CELLS, MATCH_TABLE, MAX_FEATURES, PHASE_CORRELATE_MAX, POSE_GRAPH_CHUNK_BYTES,
                   POSE_GRAPH_MAX_GRAPHS, POSE_GRAPH_MAX_ITERATIONS, POSE_GRAPH_MAX_TRIALS, POSE_GRAPH_MAX_VERTICES, POSE_GRAPH_STATS,
                   PRIOR_MAX_LINEAR, PRIOR_RECORD, ROAM_E_ARG, ROAM_E_CAPACITY, ROAM_E_HIP, ROAM_E_NODEVICE, ROAM_E_STATE, ROAM_OK,
                   SCAN_CONTEXT_MAX_CLIP, SCAN_CONTEXT_MAX_RINGS, SCAN_CONTEXT_MAX_ROWS, SCAN_CONTEXT_MAX_SECTORS, STEP_NEW_SEQUENCE,
                   TIME_DFT_FIVE, TIME_FFT_COLS, TIME_FFT_FIVE, TIME_FFT_ROWS, TIME_FFT_TRANSPOSE, WARP_AFFINE_INVERSE_MAP,
                   WARP_AFFINE_MAX_COORD, WARP_AFFINE_MAX_SIDE, WARP_POLAR_INVERSE, WARP_POLAR_LOG, AutoPriorCfg, EngineCfg, IcpOpts,
                   IcpStats, KeyframeHdr, LaneResult, PoseGraphOpts, RoamError, _INTERNAL_SIGS, _P, _SIGS, _vp)
from ._args import (_batch_operands, _batch_strides, _f32_rows_in_place, _int_in, auto_prior_args, fmt_cart_radius, fmt_clip_radius,
                    fmt_register_batch_args, fmt_rotation_batch_args, icp2d_args, icp2d_opts, invert_affine, klt_flow_args,
                    loop_cloud_args, loop_cloud_points, loop_map_args, loop_motion_args, loop_offsets_args, loop_query_args, loop_verify_args,
                    map_field_args, map_field_table_args, map_match_clouds, map_match_indices, map_match_priors, map_match_window,
                    motion_prior_args, peak_conditions, phase_correlate_args, pose_graph_args, scan_context_floor, warp_affine_args)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ROAM_LIB") or os.path.join(_HERE, "csrc", "libroam_hip.so")     # ROAM_LIB: an A/B build (profiles/build_variant.py)
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
        if not _int_in(v):
            raise ValueError(f"scan context: {name} is an integer, not {v!r}")
    if clip_px is not None and not _int_in(clip_px):
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


def scan_context_images(polar, clip_px, sectors, rings):
    """the image operand of the describing entries -> (a3, n, rows, cols, row_stride, image_stride, clip): a 2-D image or a 3-D batch
    of float32, read in place where its strides allow (_f32_rows_in_place).  ValueError as scan_context_plan"""
    a = np.asarray(polar)
    if a.ndim not in (2, 3) or a.size == 0:
        raise ValueError(f"scan context: a 2-D image or a 3-D batch, not shape {a.shape}")
    a3, n, rows, cols, row_stride, image_stride = _batch_strides(_f32_rows_in_place(a))
    clip, _, _ = scan_context_plan(rows, cols, clip_px, sectors, rings)
    return a3, n, rows, cols, row_stride, image_stride, clip


def scan_context_offset_table(rows, sectors):
    """roam_scan_context_offset_table, host code only (no device, no context): the tables of the origin-shifted descriptor by the
    host's libm -> (cos, sin of the row centres (rows,), cos, sin of the sector boundaries (sectors,)) float64.  ValueError outside
    scan_context_plan's limits"""
    for name, v in (("rows", rows), ("sectors", sectors)):
        if not _int_in(v):
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
    if not _int_in(rows, 1, SCAN_CONTEXT_MAX_ROWS):
        raise ValueError(f"loop db: rows an integer in [1, {SCAN_CONTEXT_MAX_ROWS}], not {rows!r}")
    c, s = np.empty(rows, np.float64), np.empty(rows, np.float64)
    if load_library().roam_polar_cloud_table(int(rows), _ptr(c), _ptr(s)) != ROAM_OK:
        raise ValueError(f"loop db: roam_polar_cloud_table refused rows {rows}")
    return c, s


def cloud_motion_table(rows, velocities, period=0.25):
    """roam_cloud_motion_table, host code only (no device, no context): the table a cloud-keeping loop database compensates a scan's
    motion with -> (n, rows, 4) float64, C S DX DY of every azimuth row: tau_t = period ((2 t - rows) / (2 rows)), (C, S) = (cos, sin)
    of vtheta tau_t by the host's libm, (DX, DY) = (vx, vy) tau_t.  velocities: (3,) -> n = 1, (n, 3), or a sequence with None
    entries; a scan without a velocity (None, or NaN in vx) has rows of NaN.  ValueError: rows no integer in [1, 65536], and what
    loop_motion_args refuses"""
    if not _int_in(rows, 1, SCAN_CONTEXT_MAX_ROWS):
        raise ValueError(f"loop db: rows an integer in [1, {SCAN_CONTEXT_MAX_ROWS}], not {rows!r}")
    if velocities is None:
        raise ValueError("loop db: cloud_motion_table needs velocities")
    if not isinstance(velocities, np.ndarray):
        velocities = list(velocities)
    one = len(velocities) == 3 and all(isinstance(c, numbers.Real) for c in velocities)       # (vx, vy, vtheta) itself
    n = 1 if one else len(velocities)
    v, period = loop_motion_args(velocities, period, n)
    out = np.empty((n, rows, 4), np.float64)
    if load_library().roam_cloud_motion_table(int(rows), period, n, _ptr(v), _ptr(out)) != ROAM_OK:
        raise ValueError(f"loop db: roam_cloud_motion_table refused rows {rows}, period {period}, velocities {v.tolist()}")
    return out


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


def map_field_table(sigma_cells=1.0, radius_cells=2):
    """roam_map_field_table, host code only (no device, no context): the smear of a match field -> (2 r + 1, 2 r + 1) uint8,
    T[dv + r][du + r] = floor(255 exp(-(du du + dv dv) / (2 sigma sigma)) + 0.5) by the host's libm.  ValueError: sigma not finite or
    <= 0, radius no integer in [0, MAP_MATCH_MAX_RADIUS]"""
    sigma, r = map_field_table_args(sigma_cells, radius_cells)
    t = np.empty((2 * r + 1, 2 * r + 1), np.uint8)
    if load_library().roam_map_field_table(sigma, r, _ptr(t)) != ROAM_OK:
        raise ValueError(f"map field: roam_map_field_table refused sigma {sigma}, radius {r}")
    return t


def map_match_angles(priors, n_theta, step_rad):
    """roam_map_match_angles, host code only: priors (3,) or (n, 3) rows x, y, theta -> (n, n_theta, 2) float64 rows (cos th_i, sin th_i)
    by the host's libm, th_i = th0 + float(i - (n_theta - 1) / 2) * step_rad - what a match multiplies with"""
    n = 1 if np.shape(priors) == (3,) else len(priors)
    p = map_match_priors(priors, n, (n_theta, step_rad, 0, 0))
    cs = np.empty((n, int(n_theta), 2), np.float64)
    if load_library().roam_map_match_angles(n, _ptr(p), int(n_theta), float(step_rad), _ptr(cs)) != ROAM_OK:
        raise ValueError(f"map match: roam_map_match_angles refused n_theta {n_theta}, step_rad {step_rad}")
    return cs


def map_match_plan(cu_count, n_query, window):
    """roam_map_match_plan, host code only: how a match of n_query queries over the raw window (n_theta, step_rad, kx, ky) is cut on a
    device of cu_count compute units -> (rows of shift per workgroup, blocks of rows): one workgroup per query, angle and block.  The
    cut changes no result"""
    p = map_match_priors((0.0, 0.0, 0.0), n_query, window)
    if not _int_in(cu_count, 1, 2 ** 31 - 1):
        raise ValueError(f"map match: cu_count an integer >= 1, not {cu_count!r}")
    rows, n_blk = C.c_int32(0), C.c_int32(0)
    if load_library().roam_map_match_plan(int(cu_count), len(p), int(window[0]), int(window[2]), int(window[3]), C.byref(rows), C.byref(n_blk)) != ROAM_OK:
        raise ValueError(f"map match: roam_map_match_plan refused {n_query} queries, window {window!r}")
    return rows.value, n_blk.value


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
        batch = a.ndim == 3
        a3, n, rows, cols, row_stride, image_stride = _batch_strides(_f32_rows_in_place(a, batches=False), lone_row_packed=True)
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
        batch = a.ndim == 3
        a3, n, rows, cols, row_stride, image_stride = _batch_strides(_f32_rows_in_place(a, batches=False), lone_row_packed=True)
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


def _candidate_slots(m, k, variant=False, verified=False):
    """the (m, k) outputs of a loop query in the order its entries take them: index, distance, shift[, variant][, poses (m, k, 3),
    stats]"""
    out = [np.empty((m, k), np.int32), np.empty((m, k), np.float64), np.empty((m, k), np.int32)]
    if variant:
        out.append(np.empty((m, k), np.int32))
    if verified:
        out += [np.empty((m, k, 3), np.float64), np.zeros((m, k), ICP_STATS)]
    return tuple(out)


def _full_arrays(m, count, want, variant=False):
    """the (m, count) distance and shift[, variant] of a loop query to every entry; not wanted: None for each"""
    dtypes = (np.float64, np.int32, np.int32)[:3 if variant else 2]
    return tuple(np.empty((m, count), dt) if want else None for dt in dtypes)


class LoopDb:
    """A database of scan-context descriptors in HBM (roam_loop_db): add, then query.  Bound to the context it was made on (None: the
    default context, asked for after the arguments have passed).  After keep_clouds every described scan also stores its polar peak
    cloud in metres, and verify / query_verify run the ICP of Context.icp2d_batch from that store."""

    def __init__(self, ctx, capacity: int, sectors: int = 60, rings: int = 20):
        for name, v, lo, hi in (("capacity", capacity, 1, 2 ** 31 - 1), ("sectors", sectors, 2, SCAN_CONTEXT_MAX_SECTORS),
                                ("rings", rings, 1, SCAN_CONTEXT_MAX_RINGS)):
            if not _int_in(v, lo, hi):
                raise ValueError(f"loop db: {name} an integer in [{lo}, {hi}], not {v!r}")
        per = sectors * (4 * rings + 8 * ((rings + 3) & ~3) + 4)
        if capacity > LOOP_DB_BYTES // per:
            raise ValueError(f"loop db: capacity at most {LOOP_DB_BYTES // per} ({per} bytes per entry, {LOOP_DB_BYTES} in all), not {capacity}")
        ctx = ctx or default_context()
        self.ctx, self.capacity, self.sectors, self.rings = ctx, int(capacity), int(sectors), int(rings)
        h = _vp()
        ctx.check(ctx.lib.roam_loop_db_create(ctx.h, self.capacity, self.sectors, self.rings, C.byref(h)))
        self.h = h
        self.cloud_rows = self.max_points = self.range_resolution_m = None      # set by keep_clouds
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

    def add_f32(self, polar, clip_px=None, floor=0.0, velocities=None, period=0.25):
        """describe a 2-D float32 polar image or a 3-D batch on the device and append -> the index of the first new entry.
        velocities (a database that keeps clouds): the scans' velocities (vx, vy, vtheta) in m/s, m/s, rad/s - (3,) for one image,
        (n, 3) or a sequence with None entries for a batch; the stored clouds are motion-compensated over the scan period
        (cloud_motion_table, roam_loop_db_add_f32_motion).  None: the plain clouds, and period is not read"""
        a3, n, rows, cols, row_stride, image_stride, _ = scan_context_images(polar, clip_px, self.sectors, self.rings)
        floor = scan_context_floor(floor)
        v, period = loop_motion_args(velocities, period, n, self.cloud_rows is not None, cols, self.range_resolution_m)
        first = C.c_int32(-1)
        if v is None:
            self.ctx.check(self.ctx.lib.roam_loop_db_add_f32(self.ctx.h, self.h, _ptr(a3), n, rows, cols, row_stride, image_stride,
                                                             int(clip_px or 0), floor, C.byref(first)))
        else:
            self.ctx.check(self.ctx.lib.roam_loop_db_add_f32_motion(self.ctx.h, self.h, _ptr(a3), n, rows, cols, row_stride, image_stride,
                                                                    int(clip_px or 0), floor, _ptr(v), period, C.byref(first)))
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
        count = len(self)
        q, m = loop_query_args(count, indices, max_index, k, max_distance)
        slots, full = _candidate_slots(len(q), k), _full_arrays(len(q), count, want_full)
        self.ctx.check(self.ctx.lib.roam_loop_db_query(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance),
                                                       *map(_ptr, slots + full)))
        return slots + full if want_full else slots

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
        if not (_int_in(index, 0) and index < len(self)):
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
        count = len(self)
        q, m = loop_query_args(count, indices, max_index, k, max_distance)
        slots, full = _candidate_slots(len(q), k, variant=True), _full_arrays(len(q), count, want_full, variant=True)
        self.ctx.check(self.ctx.lib.roam_loop_db_query_offsets(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance),
                                                               *map(_ptr, slots + full)))
        return slots + full if want_full else slots

    def variant_offsets(self, variant):
        """variant indices (...) -> their offsets in metres (..., 2); variant 0 (and a database without offsets) is (0, 0)"""
        table = np.zeros((1, 2)) if self.offsets_m is None else np.concatenate([np.zeros((1, 2)), self.offsets_m])
        return table[np.asarray(variant)]

    def query_verify_offsets(self, indices, max_index, k=8, max_distance=np.inf, opts=None):
        """roam_loop_db_query_verify_offsets: query_verify plus the winning variants (m, k) int32 before the poses"""
        self._needs_clouds()
        o = icp2d_opts(opts)
        q, m = loop_query_args(len(self), indices, max_index, k, max_distance)
        slots = _candidate_slots(len(q), k, variant=True, verified=True)
        self.ctx.check(self.ctx.lib.roam_loop_db_query_verify_offsets(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance),
                                                                      C.byref(o), *map(_ptr, slots)))
        return slots

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
        self.cloud_rows, self.max_points, self.range_resolution_m = rows, mp, res

    def _needs_clouds(self):
        if self.cloud_rows is None:
            raise ValueError("loop db: keeps no clouds (keep_clouds)")

    def set_cloud(self, index, xy):
        """replace the cloud of the stored entry `index` by xy (n, 2) metres, n <= max_points"""
        self._needs_clouds()
        a = loop_cloud_points(xy, self.max_points)
        index = self._entry(index)
        self.ctx.check(self.ctx.lib.roam_loop_db_set_cloud(self.ctx.h, self.h, index, _ptr(a), len(a)))

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
        index = self._entry(index)
        xy = np.empty((self.max_points, 2), np.float64)
        n, n_peaks = C.c_int32(0), C.c_int32(0)
        self.ctx.check(self.ctx.lib.roam_loop_db_get_cloud(self.ctx.h, self.h, index, _ptr(xy), self.max_points, C.byref(n), C.byref(n_peaks)))
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
        slots = _candidate_slots(len(q), k, verified=True)
        self.ctx.check(self.ctx.lib.roam_loop_db_query_verify(self.ctx.h, self.h, len(q), _ptr(q), _ptr(m), int(k), float(max_distance), C.byref(o),
                                                              *map(_ptr, slots)))
        return slots

    # ---- the global map
    def map_bounds(self, poses, use=None):
        """roam_loop_db_map_bounds: (bounds (4,) float64 = min x, max x, min y, max y of the used entries' points at these poses, their
        number); no point: (+inf, -inf, +inf, -inf), 0"""
        self._needs_clouds()
        p, u, _, _, _, _ = loop_map_args(len(self), poses, use)
        b, n = np.empty(4, np.float64), C.c_int64(0)
        self.ctx.check(self.ctx.lib.roam_loop_db_map_bounds(self.ctx.h, self.h, _ptr(p), _ptr(u), _ptr(b), C.byref(n)))
        return b, n.value

    def _map_args(self, poses, use, res, extent, min_hits, min_views):
        """loop_map_args for the entries that need an extent: ValueError for None"""
        args = loop_map_args(len(self), poses, use, res, extent, min_hits, min_views)
        if args[3] is None:
            raise ValueError("global map: extent (ox, oy, W, H), not None")
        return args

    def map_render(self, poses, res, extent, min_hits=1, min_views=1, use=None, grids=True, cap=None):
        """roam_loop_db_map_render on the extent (ox, oy, W, H) -> dict: hits, views (H, W) uint32 (None without grids), points (M, 2)
        float64, point_hits, point_views (M,) uint32, outside.  cap (None: as many as there can be - the cells, or the used entries'
        points if those are fewer): more map points than that raise RoamError ROAM_E_CAPACITY, its .required the count"""
        self._needs_clouds()
        p, u, res, (ox, oy, W, H), min_hits, min_views = self._map_args(poses, use, res, extent, min_hits, min_views)
        if cap is None:
            n = self.cloud_counts()[0].astype(np.int64)
            cap = int(min(W * H, n.sum() if u is None else n[u != 0].sum()))
        if not _int_in(cap, 0, 2 ** 31 - 1):
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
        p, u, res, extent, min_hits, min_views = self._map_args(poses, use, res, extent, min_hits, min_views)
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


def _match_outputs(n, window, volume):
    n_theta, _, kx, ky = window
    return (np.empty((n, 3), np.float64), np.empty((n, 6), np.int32),
            np.empty((n, n_theta, 2 * ky + 1, 2 * kx + 1), np.uint32) if volume else None)


class MapField:
    """The match field of a rendered global map, resident in HBM (roam_map_field): one byte per cell, the occupied cells (hits >=
    min_hits and views >= min_views) smeared with `table` (None: map_field_table(sigma_cells, radius)) by a maximum.  Bound to the
    context it was made on (None: the default context, asked for after the arguments have passed)."""

    def __init__(self, ctx, hits, views, origin, cell_m, min_hits=1, min_views=1, sigma_cells=1.0, radius=2, table=None):
        h, v, ox, oy, res, W, H, min_hits, min_views, radius, table = map_field_args(hits, views, origin, cell_m, min_hits, min_views, radius, table)
        if table is None:
            table = map_field_table(sigma_cells, radius)
        ctx = ctx or default_context()
        self.ctx, self.origin, self.cell_m, self.shape, self.radius, self.table = ctx, (ox, oy), res, (H, W), radius, table
        f = _vp()
        ctx.check(ctx.lib.roam_map_field_create(ctx.h, ox, oy, res, W, H, _ptr(h), _ptr(v), min_hits, min_views, radius, _ptr(table), C.byref(f)))
        self.h = f

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.roam_map_field_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read(self):
        """-> the field, (H, W) uint8"""
        out = np.empty(self.shape, np.uint8)
        self.ctx.check(self.ctx.lib.roam_map_field_read(self.ctx.h, self.h, _ptr(out)))
        return out

    def match_clouds(self, clouds, priors, window, volume=False):
        """roam_map_match_clouds: clouds (one (n, 2) array or a sequence, metres in the sensor frame) at priors ((3,) or (n, 3) rows x, y,
        theta) over the raw window (n_theta, step_rad, kx, ky) -> (poses (n, 3) float64, info (n, 6) int32: score, i, b, a, n_points,
        n_inside, the score volume (n, n_theta, 2 ky + 1, 2 kx + 1) uint32 or None)"""
        xy, offsets = map_match_clouds(clouds)
        p = map_match_priors(priors, len(offsets) - 1, window, volume)
        out = _match_outputs(len(p), window, volume)
        self.ctx.check(self.ctx.lib.roam_map_match_clouds(self.ctx.h, self.h, len(p), _ptr(xy), _ptr(offsets), _ptr(p), int(window[0]), float(window[1]),
                                                          int(window[2]), int(window[3]), *map(_ptr, out)))
        return out

    def match_db(self, db, indices, priors, window, volume=False):
        """roam_loop_db_map_match: the same with the resident clouds of the entries `indices` (None: the newest) of a LoopDb that keeps
        clouds; no cloud crosses the host"""
        db._needs_clouds()
        if db.ctx is not self.ctx:
            raise ValueError("map match: the database and the field were made on different contexts")
        idx = map_match_indices(len(db), indices)
        p = map_match_priors(priors, len(idx), window, volume)
        out = _match_outputs(len(p), window, volume)
        self.ctx.check(self.ctx.lib.roam_loop_db_map_match(self.ctx.h, db.h, self.h, len(p), _ptr(idx), _ptr(p), int(window[0]), float(window[1]),
                                                           int(window[2]), int(window[3]), *map(_ptr, out)))
        return out

    def time_match(self, hits, views, clouds, priors, window, min_hits=1, min_views=1, reps=5):
        """(field build ms, match ms) per launch (roam_time_map_match): the build of this field from hits / views into scratch, and the
        match kernels of this call on the resident field"""
        h, v, _, _, _, W, H, min_hits, min_views, _, _ = map_field_args(hits, views, self.origin, self.cell_m, min_hits, min_views, self.radius)
        if (H, W) != self.shape:
            raise ValueError(f"map field: hits and views {(H, W)}, the field is {self.shape}")
        xy, offsets = map_match_clouds(clouds)
        p = map_match_priors(priors, len(offsets) - 1, window)
        ms = (C.c_float * 2)()
        self.ctx.check(self.ctx.lib.roam_time_map_match(self.ctx.h, self.h, _ptr(h), _ptr(v), min_hits, min_views, self.radius, _ptr(self.table), len(p),
                                                        _ptr(xy), _ptr(offsets), _ptr(p), int(window[0]), float(window[1]), int(window[2]),
                                                        int(window[3]), int(reps), ms))
        return tuple(float(t) for t in ms)


def match_table(poses, info):
    """the two outputs of a match -> MATCH_TABLE rows: fraction = score / (255 n_points) (0 without points), found = score > 0"""
    t = np.zeros(len(poses), MATCH_TABLE)
    t["x"], t["y"], t["theta"] = poses[:, 0], poses[:, 1], poses[:, 2]
    t["score"], t["i"], t["b"], t["a"], t["nPoints"], t["nInside"] = (info[:, k] for k in range(6))
    t["fraction"] = np.where(info[:, 4] > 0, info[:, 0] / (255.0 * np.maximum(info[:, 4], 1)), 0.0)
    t["found"] = info[:, 0] > 0
    return t


def default_context(device_id: int = None) -> Context:
    """Process-wide context per device (lazily created); device from ROAM_DEVICE / LOCAL_RANK."""
    if device_id is None:
        device_id = int(os.environ.get("ROAM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _lock:
        if device_id not in _default:
            _default[device_id] = Context(device_id)
        return _default[device_id]
