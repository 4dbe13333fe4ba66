"""The argument checks and operand packing of the binding (_ffi.py) that make no library call: each raises before anything reaches
libroam_hip.so, and all of it runs where the library is not built."""
import numbers

import numpy as np

from ._abi import (FMT_MAX_COLS, FMT_MAX_R, FMT_MAX_ROWS, FMT_MIN_R, ICP_DEFAULTS, ICP_ITERATION_LIMIT, ICP_MAX_COORD, ICP_MAX_PAIRS,
                   ICP_MAX_POINTS, KLT_MAX_GUESS, LOOP_DB_BYTES, LOOP_MAX_K, LOOP_MAX_OFFSETS, MAP_MATCH_MAX_ANGLES, MAP_MATCH_MAX_QUERIES,
                   MAP_MATCH_MAX_RADIUS, MAP_MATCH_MAX_SHIFT, MAP_MATCH_MAX_VOLUME, MAP_MAX_CELLS, PHASE_CORRELATE_MAX,
                   POSE_GRAPH_MAX_GRAPHS, POSE_GRAPH_MAX_ITERATIONS, POSE_GRAPH_MAX_TRIALS, POSE_GRAPH_MAX_VERTICES, PRIOR_MAX_LINEAR,
                   SCAN_CONTEXT_MAX_ROWS, WARP_AFFINE_MAX_COORD, WARP_AFFINE_MAX_SIDE, AutoPriorCfg, IcpOpts, PoseGraphOpts)


def _int_in(v, lo=None, hi=None):
    """an integer, not a bool, with lo <= v <= hi (None: no bound on that side)"""
    return isinstance(v, numbers.Integral) and not isinstance(v, bool) and (lo is None or lo <= v) and (hi is None or v <= hi)


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


def scan_context_floor(floor):
    """the float floor of the describing entries: finite and >= 0 (ValueError otherwise)"""
    if not isinstance(floor, numbers.Real) or isinstance(floor, bool) or not np.isfinite(floor) or floor < 0:
        raise ValueError(f"scan context: floor finite and >= 0, not {floor!r}")
    return float(floor)


def loop_query_args(count, indices, max_index, k, max_distance):
    """the checks of LoopDb.query before any library call -> (query_index, max_index) int32 arrays"""
    q = np.ascontiguousarray(indices, np.int32).ravel()
    m = np.ascontiguousarray(max_index, np.int32).ravel()
    if len(q) < 1 or len(q) != len(m):
        raise ValueError(f"loop query: query indices and max_index of one length >= 1, not {len(q)} and {len(m)}")
    if q.min() < 0 or q.max() >= count:
        raise ValueError(f"loop query: query indices in [0, {count})")
    if not _int_in(k, 1, LOOP_MAX_K):
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


def loop_cloud_args(capacity, rows, max_points, point_stride, range_resolution_m):
    """the checks of LoopDb.keep_clouds before any library call -> (rows, max_points, point_stride, range_resolution_m)"""
    if not _int_in(rows, 1, SCAN_CONTEXT_MAX_ROWS):
        raise ValueError(f"loop db: rows an integer in [1, {SCAN_CONTEXT_MAX_ROWS}], not {rows!r}")
    if not _int_in(max_points, 1, ICP_MAX_POINTS):
        raise ValueError(f"loop db: max_points an integer in [1, {ICP_MAX_POINTS}], not {max_points!r}")
    if not _int_in(point_stride, 1, 2 ** 31 - 1):
        raise ValueError(f"loop db: point_stride an integer >= 1, not {point_stride!r}")
    res = range_resolution_m
    if not isinstance(res, numbers.Real) or isinstance(res, bool) or not np.isfinite(res) or not res > 0:
        raise ValueError(f"loop db: range_resolution_m finite and > 0, not {res!r}")
    if capacity * max_points * 16 > LOOP_DB_BYTES:
        raise ValueError(f"loop db: capacity {capacity} x max_points {max_points} x 16 bytes is beyond the {LOOP_DB_BYTES} bytes of a database")
    return int(rows), int(max_points), int(point_stride), float(res)


def loop_motion_args(velocities, period, n, keeps_clouds=True, cols=None, range_resolution_m=None):
    """the checks of the velocities of an add of n scans (LoopDb.add_f32, Engine.loop_db_add, Engine.time_loop_cloud) and of
    cloud_motion_table before any library call -> (velocities (n, 3) float64 rows (vx, vy, vtheta), C order, or None; period).
    velocities: None (no motion compensation: period is not read), one (3,) velocity for a single scan, an (n, 3) array in which a
    NaN vx marks a scan without a velocity, or a sequence of n entries, each (3,) or None.  ValueError: velocities for a database
    that keeps no clouds, a period that is not finite or <= 0, a wrong shape, a component that is not finite, a velocity for which
    hypot(vx, vy) period / 2 plus the largest range cols range_resolution_m exceeds 1e6 m (checked when both are given)"""
    if velocities is None:
        return None, 0.25
    if not keeps_clouds:
        raise ValueError("loop db: velocities for a database that keeps no clouds (keep_clouds)")
    if not isinstance(period, numbers.Real) or isinstance(period, bool) or not np.isfinite(period) or not period > 0:
        raise ValueError(f"loop db: period finite and > 0, not {period!r}")
    if isinstance(velocities, np.ndarray):
        v = velocities.reshape(1, 3) if velocities.shape == (3,) else velocities
        if v.dtype.kind not in "fiu" or v.shape != (n, 3):
            raise ValueError(f"loop db: velocities ({n}, 3) numbers, rows (vx, vy, vtheta), not {v.dtype} {velocities.shape}")
        out = np.array(v, np.float64, order="C")
    else:
        v = list(velocities)
        if len(v) == 3 and all(isinstance(c, numbers.Real) and not isinstance(c, bool) for c in v):
            v = [v]                                   # one velocity, not three scans
        if len(v) != n:
            raise ValueError(f"loop db: {len(v)} velocities for {n} scans")
        out = np.full((n, 3), np.nan)
        for i, row in enumerate(v):
            if row is None:
                continue
            r = np.asarray(row)
            if r.shape != (3,) or r.dtype.kind not in "fiu":
                raise ValueError(f"loop db: velocities[{i}] is (vx, vy, vtheta) or None, not {row!r}")
            if np.isnan(r[0]):
                raise ValueError(f"loop db: velocities[{i}] = {row!r} is not finite (None: no velocity)")
            out[i] = r
    moving = ~np.isnan(out[:, 0])
    bad = np.flatnonzero(moving & ~np.isfinite(out).all(axis=1))
    if bad.size:
        raise ValueError(f"loop db: velocities[{int(bad[0])}] = {out[bad[0]].tolist()} is not finite")
    if cols is not None and range_resolution_m is not None:
        reach = np.hypot(out[:, 0], out[:, 1]) * float(period) / 2.0 + cols * range_resolution_m
        bad = np.flatnonzero(moving & ~(reach <= ICP_MAX_COORD))
        if bad.size:
            raise ValueError(f"loop db: velocities[{int(bad[0])}] = {out[bad[0]].tolist()} over {period} s moves a point at "
                             f"{cols * range_resolution_m:g} m beyond {ICP_MAX_COORD:g} m")
    return out, float(period)


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
        if not all(_int_in(v, 1) for v in (W, H)):
            raise ValueError(f"global map: extent W and H integers >= 1, not {W!r} and {H!r}")
        if W * H > MAP_MAX_CELLS:
            raise ValueError(f"global map: extent W H = {W * H} cells, more than {MAP_MAX_CELLS}")
        extent = (float(ox), float(oy), int(W), int(H))
    for name, v in (("min_hits", min_hits), ("min_views", min_views)):
        if not _int_in(v, 1, 2 ** 31 - 1):
            raise ValueError(f"global map: {name} an integer >= 1, not {v!r}")
    return p, use, float(res), extent, int(min_hits), int(min_views)


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and np.isfinite(v)


def map_field_table_args(sigma_cells, radius_cells):
    """the checks of map_field_table before any library call -> (sigma, radius)"""
    if not (_real(sigma_cells) and sigma_cells > 0):
        raise ValueError(f"map field: sigmaCells finite and > 0, not {sigma_cells!r}")
    if not _int_in(radius_cells, 0, MAP_MATCH_MAX_RADIUS):
        raise ValueError(f"map field: radiusCells an integer in [0, {MAP_MATCH_MAX_RADIUS}], not {radius_cells!r}")
    return float(sigma_cells), int(radius_cells)


def map_field_args(hits, views, origin, cell_m, min_hits=1, min_views=1, radius=2, table=None):
    """the checks of MapField before any library call -> (hits, views (H, W) uint32 C order, ox, oy, res, W, H, min_hits, min_views,
    radius, table (2 radius + 1, 2 radius + 1) uint8 or None when none was given)"""
    if hits is None or views is None:
        raise ValueError("map field: a map rendered with its grids (grids=True), not hits / views = None")
    h, v = np.asarray(hits), np.asarray(views)
    if h.dtype.kind not in "iu" or v.dtype.kind not in "iu" or h.ndim != 2 or h.shape != v.shape or h.size == 0:
        raise ValueError(f"map field: hits and views two (H, W) integer grids of one shape, not {h.dtype} {h.shape} and {v.dtype} {v.shape}")
    if h.size > MAP_MAX_CELLS:
        raise ValueError(f"map field: W H = {h.size} cells, more than {MAP_MAX_CELLS}")
    if (h.dtype != np.uint32 and (h.min() < 0 or h.max() >= 2 ** 32)) or (v.dtype != np.uint32 and (v.min() < 0 or v.max() >= 2 ** 32)):
        raise ValueError("map field: hits and views of counts in [0, 2^32)")
    if len(origin) != 2 or not all(_real(o) for o in origin):
        raise ValueError(f"map field: origin (ox, oy) finite, not {origin!r}")
    if not (_real(cell_m) and cell_m > 0):
        raise ValueError(f"map field: cellM finite and > 0, not {cell_m!r}")
    for name, t in (("minHits", min_hits), ("minViews", min_views)):
        if not _int_in(t, 1, 2 ** 31 - 1):
            raise ValueError(f"map field: {name} an integer >= 1, not {t!r}")
    if not _int_in(radius, 0, MAP_MATCH_MAX_RADIUS):
        raise ValueError(f"map field: radiusCells an integer in [0, {MAP_MATCH_MAX_RADIUS}], not {radius!r}")
    if table is not None:
        t = np.asarray(table)
        if t.dtype != np.uint8 or t.shape != (2 * radius + 1, 2 * radius + 1):
            raise ValueError(f"map field: table ({2 * radius + 1}, {2 * radius + 1}) uint8, not {t.dtype} {t.shape}")
        table = np.ascontiguousarray(t)
    H, W = h.shape
    return (np.ascontiguousarray(h, np.uint32), np.ascontiguousarray(v, np.uint32), float(origin[0]), float(origin[1]), float(cell_m), int(W), int(H),
            int(min_hits), int(min_views), int(radius), table)


def map_match_window(cell_m, reach_m=3.0, reach_rad=0.12, step_rad=0.01):
    """MapLocalizer.match's window in metres and radians -> (n_theta, step_rad, kx, ky): k = floor(reach / cellM + 1e-9) cells to either
    side, reachM a scalar or (x, y); n_theta = 2 floor(reachRad / stepRad + 1e-9) + 1 (reachRad = 0: the prior's angle alone).
    ValueError: a reach that is not finite or < 0, more than MAP_MATCH_MAX_SHIFT cells or MAP_MATCH_MAX_ANGLES angles, stepRad not
    finite or <= 0 with a reachRad > 0"""
    rx, ry = (reach_m, reach_m) if isinstance(reach_m, numbers.Real) else (tuple(reach_m) if len(reach_m) == 2 else (None, None))
    if not (_real(rx) and _real(ry) and rx >= 0 and ry >= 0):
        raise ValueError(f"map match: reachM a finite scalar or (x, y) >= 0, not {reach_m!r}")
    kx, ky = int(np.floor(rx / cell_m + 1e-9)), int(np.floor(ry / cell_m + 1e-9))
    if kx > MAP_MATCH_MAX_SHIFT or ky > MAP_MATCH_MAX_SHIFT:
        raise ValueError(f"map match: reachM {reach_m!r} at cellM {cell_m} is ({kx}, {ky}) cells, more than {MAP_MATCH_MAX_SHIFT}")
    if not (_real(reach_rad) and reach_rad >= 0):
        raise ValueError(f"map match: reachRad finite and >= 0, not {reach_rad!r}")
    if not (_real(step_rad) and step_rad >= 0) or (step_rad == 0 and reach_rad > 0):
        raise ValueError(f"map match: stepRad finite and > 0, not {step_rad!r}")
    half = int(np.floor(reach_rad / step_rad + 1e-9)) if reach_rad > 0 else 0
    if 2 * half + 1 > MAP_MATCH_MAX_ANGLES:
        raise ValueError(f"map match: reachRad {reach_rad} at stepRad {step_rad} is {2 * half + 1} angles, more than {MAP_MATCH_MAX_ANGLES}")
    return 2 * half + 1, float(step_rad), kx, ky


def map_match_priors(priors, n, window, volume=False):
    """priors (3,) for every query or (n, 3) rows x, y, theta, and the raw window (n_theta, step_rad, kx, ky) -> priors (n, 3) float64"""
    n_theta, step_rad, kx, ky = window
    if not (_int_in(n_theta, 1, MAP_MATCH_MAX_ANGLES) and n_theta % 2 == 1):
        raise ValueError(f"map match: n_theta an odd integer in [1, {MAP_MATCH_MAX_ANGLES}], not {n_theta!r}")
    if not (_real(step_rad) and step_rad >= 0):
        raise ValueError(f"map match: step_rad finite and >= 0, not {step_rad!r}")
    for name, k in (("kx", kx), ("ky", ky)):
        if not _int_in(k, 0, MAP_MATCH_MAX_SHIFT):
            raise ValueError(f"map match: {name} an integer in [0, {MAP_MATCH_MAX_SHIFT}], not {k!r}")
    if not 1 <= n <= MAP_MATCH_MAX_QUERIES:
        raise ValueError(f"map match: between 1 and {MAP_MATCH_MAX_QUERIES} queries, not {n}")
    p = np.asarray(priors)
    if p.dtype.kind not in "fiu":
        raise ValueError(f"map match: priors of numbers, not {p.dtype}")
    if p.shape == (3,):
        p = np.tile(p, (n, 1))
    if p.shape != (n, 3):
        raise ValueError(f"map match: priors (3,) or ({n}, 3) rows x, y, theta - one per query - not {p.shape}")
    p = np.ascontiguousarray(p, np.float64)
    reach = float((n_theta - 1) // 2) * step_rad
    if not (np.all(np.isfinite(p)) and np.all(np.abs(p[:, :2]) <= ICP_MAX_COORD) and np.all(np.isfinite(p[:, 2] + reach))
            and np.all(np.isfinite(p[:, 2] - reach))):
        raise ValueError(f"map match: priors with an entry that is not finite or beyond {ICP_MAX_COORD:g} m")
    if volume and n * n_theta * (2 * ky + 1) * (2 * kx + 1) > MAP_MATCH_MAX_VOLUME:
        raise ValueError(f"map match: a score volume of {n * n_theta * (2 * ky + 1) * (2 * kx + 1)} entries, more than {MAP_MATCH_MAX_VOLUME}: "
                         "fewer queries per call, or volume=False")
    return p


def map_match_clouds(clouds):
    """one (n, 2) cloud or a sequence of them, metres in the sensor frame -> (xy (total, 2) float64, offsets (n_query + 1,) int64).
    ValueError as loop_cloud_points, at most ICP_MAX_POINTS points each"""
    if isinstance(clouds, np.ndarray) and clouds.ndim == 2:
        clouds = [clouds]
    parts = [loop_cloud_points(c, ICP_MAX_POINTS) for c in clouds]
    if not parts:
        raise ValueError("map match: no cloud")
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(c) for c in parts], out=offsets[1:])
    return np.ascontiguousarray(np.concatenate(parts, axis=0)), offsets


def map_match_indices(count, indices):
    """entries of a loop database as queries (None: the newest) -> (n,) int32.  ValueError: none, or one outside [0, count)"""
    if indices is None:
        if count < 1:
            raise ValueError("map match: an empty database has no newest entry")
        return np.array([count - 1], np.int32)
    a = np.asarray(indices)
    if a.dtype.kind not in "iu" or a.size == 0:
        raise ValueError(f"map match: indices of at least one integer, not {a.dtype} {a.shape}")
    a = a.ravel()
    if a.min() < 0 or a.max() >= count:
        raise ValueError(f"map match: entry indices in [0, {count})")
    return np.ascontiguousarray(a, np.int32)


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
        if not _int_in(o[name]):
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


def _f32_rows_in_place(a, batches=True):
    """a float32 view with unit column stride and forward row / image strides is read in place; anything else is copied.
    batches=False (the warps): only a 2-D view is read in place, a 3-D batch is always made contiguous"""
    ok = a.dtype == np.float32 and a.strides[-1] == 4 and a.strides[-2] % 4 == 0 and a.strides[-2] >= 4 * a.shape[-1]
    if ok and a.ndim == 3:
        ok = batches and a.strides[0] % 4 == 0 and a.strides[0] >= (a.shape[1] - 1) * a.strides[1] + 4 * a.shape[2]
    return a if ok else np.ascontiguousarray(a, np.float32)


def _batch_strides(a, lone_row_packed=False):
    """a 2-D image promoted to a batch of one, or a 3-D batch -> (a3, n, rows, cols, row_stride, image_stride), strides in floats.
    lone_row_packed (the warps): an image of one row states row_stride = cols, whatever stride its view carries"""
    a3 = a if a.ndim == 3 else a[None]
    n, rows, cols = a3.shape
    row_stride = cols if lone_row_packed and rows <= 1 else a3.strides[1] // 4
    image_stride = a3.strides[0] // 4 if n > 1 else rows * row_stride
    return a3, n, rows, cols, row_stride, image_stride


def _batch_operands(a, b):
    """two images or two batches of one shape as the batched entries take them -> (a3, b3, n, rows, cols, row_stride, image_stride),
    strides in floats: _f32_rows_in_place on each, 2-D promoted to a batch of one"""
    a, b = _f32_rows_in_place(a), _f32_rows_in_place(b)
    a3, b3 = (a, b) if a.ndim == 3 else (a[None], b[None])
    n = a3.shape[0]
    if a3.strides[0 if n > 1 else 1:] != b3.strides[0 if n > 1 else 1:]:     # one pair of strides describes both operands
        a3, b3 = np.ascontiguousarray(a3), np.ascontiguousarray(b3)
    return (a3, b3) + _batch_strides(a3)[1:]
