"""Loop-closure candidates on the device: the radar scan context of Kim et al. (the MulRan data set).

The reference stops at a commented-out "import m2dp" (Mapping.py:7) and a Keyframe.pointCloud marked "not sure if needed"
(Mapping.py:61-62); it has no place recognition, so this module has nothing to be pinned against - its contract is
tests/scan_context_model.py.  The polar scan is area-averaged to sectors x rings; two places are compared by the mean cosine distance
of their sector columns, minimised over all circular sector shifts; the best shift is a yaw estimate (yaw of the query minus yaw of
the candidate ~ 2 pi shift / sectors).  The device compares a query with every stored keyframe at every shift exactly: no ring-key
tree, no coarse sector-key alignment.

What comes out of LoopDetector are CANDIDATES and a yaw.  The plain descriptor's reach is short: on the synthetic worlds a revisit
2.5 m off the stored place still ranks first but at 0.79 of the next place's distance, and at 5 m it is not recognised (the point
reflectors move to other rings).

Origin offsets (the augmentation of Scan Context++).  LoopDetector(originOffsetsM=offsetGrid(5.0, 2.5)) describes every added scan
again as seen from 24 virtual origins a lane width apart (csrc/loop_offset.hip; contract tests/scan_context_offset_model.py), keeps
these variants beside the entry and uses them on the QUERY side: the distance of a pair is the minimum over the query's variants
against the candidate's plain descriptor, and the winning origin o becomes the translation prior -R(yaw) o of the verification.
On the synthetic world four revisits 5 m off their place (the next lane), of which the plain descriptor ranks two first by under
4 %, all rank first (0.018-0.022 against 0.027-0.030 for the best wrong place), the winning origin is within 0.4-1.7 m of the true
displacement, and the ICP from that seed is accepted within 0.07 m where the plain seed is rejected (docs/PARITY.md).  At 7.5 m and
at 10 m the 5 m grid puts only two of four first: that is where it still fails.  The candidate side is not augmented.

Verification.  A candidate is verified metrically by a trimmed point-to-point ICP of the two keyframes' polar peak clouds
(Keyframe.pointCloud, which the reference stores and never reads), seeded with the candidate's yaw: csrc/icp.hip, every pair of a
call in one device pass; contract tests/icp_model.py.  alignPointClouds aligns clouds, verifyCandidates turns LoopDetector.query's
arrays into accepted SE(2) edges, closeLoops feeds them to PoseGraphLib.graphFromKeyframes and optimises.  The Fourier-Mellin route
(FMT.getTransformUsingFMT after a pre-rotation by the yaw) is independent of this one and not used here.

Resident clouds.  LoopDetector(keepClouds=True, rows=...) makes the database the owner of the clouds: every scan that is described
(add, Engine.loop_db_add) leaves its polar peaks in metres beside its descriptor, built on the device at that moment - an engine's
pool has forgotten the scan long before a revisit is recognised.  verify and queryAndVerify run the same ICP from that store, the
second with no host round trip between the query and the verification; closeLoops uses it when the detector keeps clouds.  The
rule of the stored points (every step-th peak, tables from the host's libm) is tests/loop_cloud_model.py.

Motion compensation.  A scan sweeps its azimuths over 0.25 s; at driving speed a cloud stored as if the sweep were instantaneous is
skewed by metres, the ICP still reports success, and the edge is 0.5 to 1.4 m off (docs/PARITY.md).  Given the scan's velocity
(add(velocity=), Engine.loop_db_add(velocities=), polarIndToLocalMetres(velocity=), closeLoops(undistort=True)) every peak is moved
to where mid-scan would have seen it while the cloud is built: MotionDistortionSolver.undistort with the time taken from the peak's
row, tests/loop_cloud_motion_model.py.  The descriptor and its origin-shifted variants are not compensated.

Global map.  The stored clouds are also what a map is made of: LoopDetector.renderMap takes one pose per entry and bins every entry's
points in the world frame on the device (csrc/loop_map.hip) -> Mapping.GlobalMap, an occupancy grid (points and distinct keyframes per
cell) and a thinned list of map points; mapFromGraph(detector, graph) is the step after closeLoops.  A closure moves every pose, so
the map is rendered again after each; nothing of it is kept in the detector.  The definition is tests/global_map_model.py.

Localisation.  GlobalMap.localizer() turns a rendered map into a resident match field, and LoopDetector.localize(localizer, indices,
priors) places stored scans in it: correlative scan-to-map matching (csrc/map_match.hip), an exhaustive search over rotations and
whole-cell shifts around a prior pose that scores every candidate against all the keyframes of the map at once - what corrects a
drifting pose between keyframes, or a second traversal after a restart, where a scan-context hit plus pairwise ICP only recognises one
stored place.  Scores are sums of bytes, so the answer is bit-reproducible; the definition is tests/map_match_model.py."""
import numbers

import numpy as np

from . import _ffi
from .parseData import RANGE_RESOLUTION_M

# verifyCandidates' default minInlierFraction: the geometric mean of the smallest true-place fraction (0.4741) and the largest
# wrong-place fraction (0.1880) that tests/icp_model.py measures on the revisit world at full density (docs/PARITY.md)
MIN_INLIER_FRACTION = 0.2985


def _yaw(shift, sectors):
    a = 2.0 * np.pi * np.asarray(shift, np.float64) / sectors
    return np.where(a > np.pi, a - 2.0 * np.pi, a)


def offsetGrid(reachM, stepM):
    """The virtual origins of LoopDetector(originOffsetsM=...): the grid of multiples of stepM within +-reachM on both axes, x-major,
    without its centre -> (n, 2) float64 metres.  offsetGrid(5.0, 2.5) is the 24 points of a 5 x 5 grid."""
    for name, v in (("reachM", reachM), ("stepM", stepM)):
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not np.isfinite(v) or not v > 0:
            raise ValueError(f"offsetGrid: {name} finite and > 0, not {v!r}")
    k = int(np.floor(reachM / stepM + 1e-9))
    if k < 1 or (2 * k + 1) ** 2 - 1 > _ffi.LOOP_MAX_OFFSETS:
        raise ValueError(f"offsetGrid: between 1 and {_ffi.LOOP_MAX_OFFSETS} points, not the {(2 * k + 1) ** 2 - 1} of reach {reachM} at step {stepM}")
    return np.array([(i * float(stepM), j * float(stepM)) for i in range(-k, k + 1) for j in range(-k, k + 1) if (i, j) != (0, 0)], np.float64)


def _seed(yaw, offsetM):
    """the ICP seed of a candidate with the yaw psi and the winning origin offset o (metres): (psi, -R(psi) o)"""
    yaw, o = np.asarray(yaw, np.float64), np.asarray(offsetM, np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([yaw, -(c * o[..., 0] - s * o[..., 1]), -(s * o[..., 0] + c * o[..., 1])], axis=-1)


def scanContext(polarImg, sectors=60, rings=20, clip_px=None, floor=0.0, originOffsetsM=None, rangeResolutionM=RANGE_RESOLUTION_M):
    """The scan-context descriptor of a float32 polar image (azimuth rows x range columns) -> (sectors, rings) float32, or of a 3-D
    batch -> (n, sectors, rings): the mean of max(value - floor, 0) over each bin, sector s = the rows [floor(s rows / sectors),
    floor((s + 1) rows / sectors)), ring r = the columns [floor(r clip / rings), floor((r + 1) clip / rings)), clip = clip_px if
    0 < clip_px < cols else cols.  floor = 0 is the plain area mean.  ValueError before the device is touched for a bad argument.
    originOffsetsM (n, 2) metres: -> (1 + n, sectors, rings), or (batch, 1 + n, sectors, rings): the plain descriptor first, then the
    scan as seen from each of these origins (x = r cos phi, y = r sin phi; tests/scan_context_offset_model.py), rangeResolutionM metres
    per range bin."""
    a = np.asarray(polarImg)
    _ffi.scan_context_images(a, clip_px, sectors, rings)          # the argument checks come before a device is asked for
    _ffi.scan_context_floor(floor)
    if originOffsetsM is not None:
        _ffi.loop_offsets_args(originOffsetsM, rangeResolutionM)
        out = _ffi.default_context().scan_context_offsets(a, originOffsetsM, rangeResolutionM, sectors, rings, clip_px, floor)
        return out[0] if a.ndim == 2 else out
    out = _ffi.default_context().scan_context(a, sectors, rings, clip_px, floor)
    return out[0] if a.ndim == 2 else out


def scanContextDistance(a, b):
    """Two descriptors of one shape -> (distance, shift, yaw): the mean cosine distance of the sector columns of a against those of b
    shifted by `shift` sectors, minimised over the shifts (the lowest shift of the minimum); yaw = 2 pi shift / sectors in (-pi, pi],
    the yaw of a's scan minus the yaw of b's.  Runs on the device through a two-entry database."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError(f"scanContextDistance: two descriptors of one (sectors, rings) shape, not {a.shape} and {b.shape}")
    db = _ffi.LoopDb(None, 2, a.shape[0], a.shape[1])
    try:
        db.add_desc(np.stack([b, a]))
        _, cd, cs = db.query([1], [1], k=1)
    finally:
        db.close()
    return float(cd[0, 0]), int(cs[0, 0]), float(_yaw(cs[0, 0], a.shape[0]))


class LoopDetector:
    """Keyframe scans in, loop-closure candidates out.  Every added scan becomes one entry (its index is its order of arrival);
    query(i) returns the k stored entries most like entry i among those at least min_gap entries older, with their distances and
    yaw differences."""

    def __init__(self, capacity, sectors=60, rings=20, clip_px=None, floor=0.0, min_gap=50, max_distance=0.2, k=8, ctx=None, keepClouds=False,
                 rows=None, maxPoints=8192, pointStride=1, rangeResolutionM=RANGE_RESOLUTION_M, originOffsetsM=None):
        """keepClouds: every added scan also stores its polar peak cloud in metres (rows: the azimuths of every scan to come; at most
        maxPoints points per entry, every step-th peak with step = max(pointStride, ceil(peaks / maxPoints))).
        originOffsetsM ((n, 2) metres, n <= 48, e.g. offsetGrid(5.0, 2.5); None: today's behaviour exactly): every added scan is also
        described as seen from these origins, a query takes the minimum distance over these variants, and the winning origin seeds the
        verification with a translation"""
        if not isinstance(min_gap, numbers.Integral) or isinstance(min_gap, bool) or min_gap < 1:
            raise ValueError(f"LoopDetector: min_gap an integer >= 1, not {min_gap!r}")
        if clip_px is not None and (not isinstance(clip_px, numbers.Integral) or isinstance(clip_px, bool) or clip_px < 0):
            raise ValueError(f"LoopDetector: clip_px a non-negative integer or None, not {clip_px!r}")
        self.floor = _ffi.scan_context_floor(floor)
        _ffi.loop_query_args(1, [0], [0], k, max_distance)
        self.clip_px, self.min_gap, self.max_distance, self.k = clip_px, int(min_gap), float(max_distance), int(k)
        self.keepClouds = bool(keepClouds)
        if self.keepClouds:
            if rows is None:
                raise ValueError("LoopDetector: keepClouds needs rows, the azimuths of the scans")
            if not isinstance(capacity, numbers.Integral) or isinstance(capacity, bool) or capacity < 1:
                raise ValueError(f"LoopDetector: capacity an integer >= 1, not {capacity!r}")
            _ffi.loop_cloud_args(capacity, rows, maxPoints, pointStride, rangeResolutionM)
        self.keepOffsets = originOffsetsM is not None
        if self.keepOffsets:
            ints = all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (capacity, sectors, rings))
            _ffi.loop_offsets_args(originOffsetsM, rangeResolutionM, *((capacity, sectors, rings) if ints else ()))
        self.db = _ffi.LoopDb(ctx, capacity, sectors, rings)
        self.sectors, self.rings = self.db.sectors, self.db.rings
        if self.keepClouds:
            self.db.keep_clouds(rows, maxPoints, pointStride, rangeResolutionM)
        if self.keepOffsets:
            self.db.keep_offsets(originOffsetsM, rangeResolutionM)

    def close(self):
        self.db.close()

    def __len__(self):
        return len(self.db)

    def add(self, polarImg, velocity=None, period=0.25):
        """describe a float32 polar image (or a 3-D batch) on the device and store it -> the index of the (first) new entry.  With
        keepClouds the image's peak cloud (all its columns) is stored too.  velocity (keepClouds): the scan's (vx, vy, vtheta) in m/s,
        m/s, rad/s, sensor frame (Keyframe.velocity) - (3,) for one image, (n, 3) for a batch, None entries allowed; the stored cloud
        is motion-compensated over the scan period (tests/loop_cloud_motion_model.py).  None: the plain cloud"""
        return self.db.add_f32(polarImg, self.clip_px, self.floor, velocity, period)

    def addDescriptors(self, desc, clouds=None):
        """store ready-made descriptors, (sectors, rings) or (n, sectors, rings) -> the index of the first new entry.  clouds (with
        keepClouds): one (K, 2) metre cloud per descriptor; without them the entries hold empty clouds"""
        if clouds is not None:
            if not self.keepClouds:
                raise ValueError("LoopDetector.addDescriptors: clouds for a detector that keeps none")
            n = 1 if np.ndim(desc) == 2 else len(desc)
            if len(clouds) != n:
                raise ValueError(f"LoopDetector.addDescriptors: {len(clouds)} clouds for {n} descriptors")
            clouds = [_ffi.loop_cloud_points(c, self.db.max_points) for c in clouds]
        first = self.db.add_desc(desc)
        for i, c in enumerate(clouds or ()):
            self.db.set_cloud(first + i, c)
        return first

    def cloud(self, i):
        """-> (xy (n, 2) float64 metres: the stored cloud of entry i, the scan's full peak count)"""
        return self.db.get_cloud(i)

    def renderMap(self, poses, cellM=0.5, extent=None, minHits=1, minViews=1, use=None, grids=True):
        """The global map of the stored clouds (keepClouds) at poses (len(self), 3) rows x, y, theta -> Mapping.GlobalMap: every
        entry's points in the world frame, binned into cells of cellM metres on the device (csrc/loop_map.hip; the definition is
        tests/global_map_model.py).  extent (ox, oy, W, H): the corner of cell (0, 0) in metres and the grid's size in cells; None:
        the points' bounding box with one cell of margin (bounds, plan, then the render; an empty map is 1 x 1 at the origin).  A
        map point is the mean position of a cell with at least minHits points from at least minViews entries.  use (len(self),): zero
        leaves an entry out.  grids=False: the two (H, W) grids are not read back"""
        from .Mapping import GlobalMap
        if not self.keepClouds:
            raise ValueError("LoopDetector.renderMap: the detector keeps no clouds (keepClouds=True)")
        p, u, res, extent, minHits, minViews = _ffi.loop_map_args(len(self.db), poses, use, cellM, extent, minHits, minViews)
        if extent is None:
            b, n = self.db.map_bounds(p, u)
            extent = _ffi.map_plan(b, res) if n else (0.0, 0.0, 1, 1)
        r = self.db.map_render(p, res, extent, minHits, minViews, u, grids)
        return GlobalMap(extent[:2], res, (extent[3], extent[2]), r["hits"], r["views"], r["points"], r["point_hits"], r["point_views"], r["outside"])

    def localize(self, localizer, indices=None, priors=(0.0, 0.0, 0.0), reachM=3.0, reachRad=0.12, stepRad=0.01, volume=False):
        """Mapping.MapLocalizer.match on the stored clouds (keepClouds) of the entries `indices` (None: the newest), which never leave
        the device: priors (3,) or (n, 3) rows x, y, theta in the map's frame, the window as there -> the _ffi.MATCH_TABLE rows, with
        volume=True also the list of score volumes"""
        if not self.keepClouds:
            raise ValueError("LoopDetector.localize: the detector keeps no clouds (keepClouds=True)")
        poses, info, scores = localizer._field.match_db(self.db, indices, priors, localizer.window(reachM, reachRad, stepRad), volume)
        return (_ffi.match_table(poses, info), list(scores)) if volume else _ffi.match_table(poses, info)

    def verify(self, queryIndex, candIndex, candYaw, candOffset=None, **verify):
        """verifyCandidates from the stored clouds: the arguments, keywords and results are verifyCandidates' without `clouds`.
        candOffset (Q, k, 2) metres, what query(withOffsets=True) returned: candidate (a, slot) is seeded with (yaw, -R(yaw) offset)
        instead of (yaw, 0, 0), and the table carries ox, oy (VERIFY_TABLE_OFFSETS)"""
        q, ci, yaw, o, accept = _verify_args(queryIndex, candIndex, candYaw, verify)
        off = None
        if candOffset is not None:
            off = np.asarray(candOffset, np.float64)
            if off.shape != ci.shape + (2,) or not np.all(np.abs(off) <= _ffi.ICP_MAX_COORD):
                raise ValueError(f"LoopDetector.verify: candOffset {ci.shape + (2,)} finite metres, not {off.shape}")
        rows, pos = _verify_rows(q, ci, len(self.db), "entries")
        if not rows:
            return [], np.zeros(0, VERIFY_TABLE if off is None else VERIFY_TABLE_OFFSETS)
        slots = [slot for _, _, slot in rows]
        offs = None if off is None else off[pos, slots]
        seeds = _seed(yaw[pos, slots], np.zeros((len(rows), 2)) if offs is None else offs)
        poses, stats = self.db.verify([r[0] for r in rows], [r[1] for r in rows], seeds, o)
        n, _ = self.db.cloud_counts()
        sizes = np.array([min(n[qi], n[cj]) for qi, cj, _ in rows])
        return _accept(len(q), rows, pos, seeds, poses, stats, sizes, *accept, offsets=offs)

    def queryAndVerify(self, indices=None, **verify):
        """query the entries `indices` (None: the newest) and verify every candidate from the stored clouds in the same device pass
        (roam_loop_db_query_verify) -> (edges, table) as verifyCandidates returns them.  A detector that keeps origin offsets queries
        over the variants and seeds every candidate with its winning offset, (yaw, -R(yaw) offset); its table carries ox, oy
        (VERIFY_TABLE_OFFSETS)"""
        idx = np.array([len(self.db) - 1], np.int32) if indices is None else np.ascontiguousarray(indices, np.int32).ravel()
        o, accept = _verify_opts(verify)
        if self.keepOffsets:
            ci, _, cs, cv, poses, stats = self.db.query_verify_offsets(idx, idx - self.min_gap + 1, self.k, self.max_distance, o)
        else:
            ci, _, cs, poses, stats = self.db.query_verify(idx, idx - self.min_gap + 1, self.k, self.max_distance, o)
        rows, pos = _verify_rows(idx, ci, len(self.db), "entries")
        if not rows:
            return [], np.zeros(0, VERIFY_TABLE_OFFSETS if self.keepOffsets else VERIFY_TABLE)
        flat = np.array([a * self.k + slot for a, (_, _, slot) in zip(pos, rows)])
        yaw = _yaw(cs, self.sectors).reshape(-1)[flat]
        offs = self.db.variant_offsets(cv.reshape(-1)[flat]) if self.keepOffsets else None
        seeds = _seed(yaw, np.zeros((len(rows), 2)) if offs is None else offs)
        n, _ = self.db.cloud_counts()
        sizes = np.array([min(n[qi], n[cj]) for qi, cj, _ in rows])
        return _accept(len(idx), rows, pos, seeds, poses.reshape(-1, 3)[flat], stats.reshape(-1)[flat], sizes, *accept, offsets=offs)

    def floorCode(self):
        """the integer floor of the u8 record form that equals this detector's floor (Engine.loop_db_add): floor * 255, which must be
        an integer in [0, 254]"""
        code = int(round(self.floor * 255.0))
        if code > 254 or abs(self.floor * 255.0 - code) > 1e-9:
            raise ValueError(f"LoopDetector: floor {self.floor} is no u8 code / 255 in [0, 254 / 255]")
        return code

    def query(self, indices=None, withOffsets=False):
        """candidates of the entries `indices` (None: the newest) among the entries j <= i - min_gap -> (index (m, k) int32, distance
        (m, k) float64, yaw (m, k) float64); unused slots hold -1, +inf, 0.  withOffsets: the distance of a pair is the minimum over
        the query's origin-shifted variants (a detector with originOffsetsM; otherwise the plain query), and a fourth array
        (m, k, 2) float64 holds the winning origin offsets in metres, (0, 0) where the plain descriptor won"""
        idx = np.array([len(self.db) - 1], np.int32) if indices is None else np.ascontiguousarray(indices, np.int32).ravel()
        if withOffsets:
            ci, cd, cs, cv = self.db.query_offsets(idx, idx - self.min_gap + 1, self.k, self.max_distance)
            return ci, cd, _yaw(cs, self.sectors), self.db.variant_offsets(cv)
        ci, cd, cs = self.db.query(idx, idx - self.min_gap + 1, self.k, self.max_distance)
        return ci, cd, _yaw(cs, self.sectors)

    def addAndQuery(self, polarImg):
        """add one image and query it -> (index, candidate indices (k,), distances (k,), yaws (k,))"""
        a = np.asarray(polarImg)
        if a.ndim != 2:
            raise ValueError(f"LoopDetector.addAndQuery: one 2-D image, not shape {a.shape}")
        i = self.add(a)
        ci, cd, yaw = self.query([i])
        return i, ci[0], cd[0], yaw[0]

    def descriptors(self):
        """the stored descriptors (n, sectors, rings) float32"""
        return self.db.get() if len(self.db) else np.empty((0, self.sectors, self.rings), np.float32)


# ---------------------------------------------------------------------------------------------------------------- verification
def polarIndToLocalMetres(pointCloud, rows, rangeResolutionM=RANGE_RESOLUTION_M, velocity=None, period=0.25):
    """The (K, 2) [thetaInd, rInd] rows of getPointCloudPolarInd -> (K, 2) float64 metres in the sensor-centred frame of
    Keyframe.featurePointsLocal: r res (cos phi, sin phi) with phi = 2 pi thetaInd / rows - (pixel - centre) resolution of the image
    convertPolarImageToCartesian makes, x along its columns and y along its rows.  Host code.
    velocity (vx, vy, vtheta) in m/s, m/s, rad/s (Keyframe.velocity): the points are motion-compensated over the scan period as the
    loop database's clouds are (tests/loop_cloud_motion_model.py): row t was seen at tau = period (2 t - rows) / (2 rows), the point
    becomes R(vtheta tau) p + (vx, vy) tau - MotionDistortionSolver.undistort with the time taken from the row"""
    pc = np.asarray(pointCloud)
    v, period = _ffi.loop_motion_args(velocity, period, 1)
    if pc.size == 0:
        return np.zeros((0, 2), np.float64)
    if pc.ndim != 2 or pc.shape[1] != 2:
        raise ValueError(f"polarIndToLocalMetres: (K, 2) rows [thetaInd, rInd], not {pc.shape}")
    if not isinstance(rows, numbers.Integral) or isinstance(rows, bool) or rows < 1:
        raise ValueError(f"polarIndToLocalMetres: rows (the azimuths of the polar image) an integer >= 1, not {rows!r}")
    pc = pc.astype(np.float64)
    phi = 2.0 * np.pi * pc[:, 0] / rows
    r = pc[:, 1] * float(rangeResolutionM)
    x0, y0 = r * np.cos(phi), r * np.sin(phi)
    if v is None or np.isnan(v[0, 0]):
        return np.stack([x0, y0], axis=1)
    tau = period * ((2.0 * pc[:, 0] - rows) / (2.0 * rows))
    a = v[0, 2] * tau
    c, s = np.cos(a), np.sin(a)
    return np.stack([((c * x0) - (s * y0)) + v[0, 0] * tau, ((s * x0) + (c * y0)) + v[0, 1] * tau], axis=1)


def _align_batch(pairs, init, opts):
    """the one device call of this module (the tests patch it) -> (poses (n, 3) rows (theta, tx, ty), stats: _ffi.ICP_STATS rows)"""
    args = _ffi.icp2d_args(pairs, init, opts)        # the argument checks come before a device is asked for
    return _ffi.default_context().icp2d_batch(pairs, args[4], args[5])


def alignPointClouds(src, dst, init=(0.0, 0.0, 0.0), **opts):
    """Trimmed point-to-point ICP of src (n, 2) onto dst (m, 2), metres, from the pose init = (theta, tx, ty) ->
    (pose (3,) (theta, tx, ty) with dst ~ R(theta) src + t, stats dict: status, iterations, n_pairs_last, n_inliers, rms).  Lists of
    clouds (one init for all, or one row each) -> (poses (N, 3), stats: a structured array with those fields), every pair in one
    device call.  opts: gate_start, gate_end, gate_decay, max_iterations, eps_trans, eps_rot, min_pairs (_ffi.ICP_DEFAULTS).  status:
    _ffi.ICP_OK, ICP_MAX_ITERATIONS or ICP_FEW_PAIRS.  ValueError before the device is touched for a bad argument."""
    one = isinstance(src, np.ndarray) and src.ndim == 2 or len(src) == 0 or np.ndim(src[0]) < 2 and np.shape(src[0]) in ((2,), (0,))
    if one:                                       # one cloud: an (n, 2) array, or a list of (x, y) rows
        poses, stats = _align_batch([(src, dst)], init, opts)
        return poses[0], {name: stats[0][name].item() for name in stats.dtype.names}
    if len(src) != len(dst):
        raise ValueError(f"alignPointClouds: {len(src)} src clouds and {len(dst)} dst clouds")
    return _align_batch(list(zip(src, dst)), init, opts)


VERIFY_TABLE = np.dtype([("query", np.int32), ("candidate", np.int32), ("slot", np.int32), ("yaw", np.float64), ("theta", np.float64),
                         ("tx", np.float64), ("ty", np.float64), ("status", np.int32), ("iterations", np.int32), ("n_pairs_last", np.int32),
                         ("n_inliers", np.int32), ("fraction", np.float64), ("rms", np.float64), ("accepted", np.bool_)])


# the table of a detector that keeps origin offsets: VERIFY_TABLE plus the winning offset of every tried candidate, metres
VERIFY_TABLE_OFFSETS = np.dtype(VERIFY_TABLE.descr + [("ox", np.float64), ("oy", np.float64)])


def verifyCandidates(clouds, queryIndex, candIndex, candYaw, *, minInlierFraction=MIN_INLIER_FRACTION, maxRmsM=None, maxTranslationM=5.0,
                     allPerQuery=False, **opts):
    """Verify loop-closure candidates by ICP and measure their edges.  clouds: one (K, 2) metre cloud per keyframe
    (polarIndToLocalMetres); queryIndex (Q,), candIndex (Q, k) and candYaw (Q, k): what went into and came out of
    LoopDetector.query - slots with index -1 are skipped.  Each candidate aligns src = clouds[query] to dst = clouds[candidate] from
    (candYaw, 0, 0), all in one device call, and is accepted when its status is OK or MAX_ITERATIONS,
    n_inliers / min(n, m) >= minInlierFraction, rms <= maxRmsM (None: gate_end) and |t| <= maxTranslationM.
    -> (edges, table).  edges: (candidate, query, (tx, ty, theta)) tuples, the measurement x_candidate^-1 x_query in the form
    PoseGraphLib.graphFromKeyframes(loopEdges=...) takes; per query the accepted candidate with the largest inlier fraction (the
    lowest rms, then the lowest slot on ties), or every accepted one with allPerQuery.  table: one row per tried candidate, a
    structured array (query, candidate, slot, yaw, theta, tx, ty, status, iterations, n_pairs_last, n_inliers, fraction, rms,
    accepted)."""
    opts.update(minInlierFraction=minInlierFraction, maxRmsM=maxRmsM, maxTranslationM=maxTranslationM, allPerQuery=allPerQuery)
    q, ci, yaw, o, accept = _verify_args(queryIndex, candIndex, candYaw, opts)
    rows, pos = _verify_rows(q, ci, len(clouds), "clouds")
    if not rows:
        return [], np.zeros(0, VERIFY_TABLE)
    seeds = np.array([[yaw[a, slot], 0.0, 0.0] for a, (_, _, slot) in zip(pos, rows)])
    poses, stats = _align_batch([(clouds[qi], clouds[cj]) for qi, cj, _ in rows], seeds, o)
    sizes = np.array([min(len(clouds[qi]), len(clouds[cj])) for qi, cj, _ in rows])
    return _accept(len(q), rows, pos, seeds, poses, stats, sizes, *accept)


def _verify_opts(keywords):
    """verifyCandidates' keywords -> (IcpOpts, (minInlierFraction, max_rms, maxTranslationM, allPerQuery)); ValueError as there"""
    kw = dict(keywords)
    minInlierFraction = kw.pop("minInlierFraction", MIN_INLIER_FRACTION)
    maxRmsM = kw.pop("maxRmsM", None)
    maxTranslationM = kw.pop("maxTranslationM", 5.0)
    allPerQuery = kw.pop("allPerQuery", False)
    o = _ffi.icp2d_opts(kw)
    max_rms = o.gate_end if maxRmsM is None else float(maxRmsM)
    if not (0.0 <= float(minInlierFraction) <= 1.0) or not max_rms >= 0.0 or not float(maxTranslationM) >= 0.0:
        raise ValueError("verifyCandidates: minInlierFraction in [0, 1], maxRmsM and maxTranslationM >= 0")
    return o, (float(minInlierFraction), max_rms, float(maxTranslationM), bool(allPerQuery))


def _verify_args(queryIndex, candIndex, candYaw, keywords):
    """-> (q (Q,), ci (Q, k), yaw (Q, k), IcpOpts, the acceptance's parameters)"""
    q = np.asarray(queryIndex).reshape(-1)
    ci = np.asarray(candIndex)
    ci = ci.reshape(len(q), -1) if ci.size else ci.reshape(len(q), 0)
    yaw = np.asarray(candYaw, np.float64).reshape(ci.shape)
    if q.dtype.kind not in "iu" or ci.dtype.kind not in "iu":
        raise ValueError("verifyCandidates: queryIndex and candIndex of integers")
    return (q, ci, yaw) + _verify_opts(keywords)


def _verify_rows(q, ci, count, what):
    """the candidates to try -> (rows: (query, candidate, slot) of every slot that holds one, pos: the row's position in q)"""
    rows = [(int(q[a]), int(ci[a, b]), b) for a in range(len(q)) for b in range(ci.shape[1]) if ci[a, b] >= 0]
    for qi, cj, _ in rows:
        if not (0 <= qi < count and cj < count):
            raise ValueError(f"verifyCandidates: query {qi} / candidate {cj} outside the {count} {what}")
    pos = np.array([a for a in range(len(q)) for b in range(ci.shape[1]) if ci[a, b] >= 0], dtype=np.int64)
    return rows, pos


def _accept(n_query, rows, pos, seeds, poses, stats, sizes, minInlierFraction, max_rms, maxTranslationM, allPerQuery, offsets=None):
    """The acceptance, written once for verifyCandidates, LoopDetector.verify and LoopDetector.queryAndVerify: the tried candidates
    (rows, pos: _verify_rows), their seeds, ICP poses and statistics, sizes = min(n, m) of each pair's clouds -> (edges, table)"""
    table = np.zeros(len(rows), VERIFY_TABLE if offsets is None else VERIFY_TABLE_OFFSETS)
    if offsets is not None:
        table["ox"], table["oy"] = offsets[:, 0], offsets[:, 1]
    table["query"], table["candidate"], table["slot"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    table["yaw"], table["theta"], table["tx"], table["ty"] = seeds[:, 0], poses[:, 0], poses[:, 1], poses[:, 2]
    for name in ("status", "iterations", "n_pairs_last", "n_inliers", "rms"):
        table[name] = stats[name]
    table["fraction"] = np.where(sizes > 0, stats["n_inliers"] / np.maximum(sizes, 1), 0.0)
    table["accepted"] = ((stats["status"] != _ffi.ICP_FEW_PAIRS) & (table["fraction"] >= minInlierFraction) & (stats["rms"] <= max_rms)
                         & (np.hypot(poses[:, 1], poses[:, 2]) <= maxTranslationM))
    edges = []
    for a in range(n_query):
        acc = [r for r in np.flatnonzero(pos == a) if table["accepted"][r]]
        if not allPerQuery and acc:
            acc = [min(acc, key=lambda r: (-table["fraction"][r], table["rms"][r], table["slot"][r]))]
        for r in acc:
            edges.append((int(table["candidate"][r]), int(table["query"][r]),
                          np.array([table["tx"][r], table["ty"][r], table["theta"][r]])))
    return edges, table


def closeLoops(keyframes, detector, clouds=None, *, rows=None, rangeResolutionM=RANGE_RESOLUTION_M, loopInformation=np.eye(3), huber=None,
               odomInformation=np.eye(3), max_iterations=20, ctx=None, undistort=False, period=0.25, **verify):
    """Close the loops of a keyframe list: keyframes with .pose and .pointCloud (Mapping.Map.keyframes) and a LoopDetector that already
    holds their scans, entry k = keyframe k.  The peak clouds are converted to metres (rows: the azimuths of the polar images, by default
    those of keyframes[0].radarPolarImg; or pass ready clouds), every keyframe is queried, the candidates are verified in one device
    call (verify: verifyCandidates' keywords and the ICP options), PoseGraphLib.graphFromKeyframes is called with the accepted edges
    and optimised.  -> (graph, edges, table); graph.get_pose(k) is keyframe k's optimised pose.  Without an accepted edge the graph is
    returned un-optimised (odometry alone has nothing to correct).  A detector that keeps clouds (LoopDetector(keepClouds=True)) and
    clouds = None: the candidates are found and verified from the detector's own store in one device pass (queryAndVerify) and
    keyframe.pointCloud, rows and rangeResolutionM are not used.  undistort=True (the path that converts keyframe.pointCloud): every
    cloud is motion-compensated with its keyframe.velocity over `period` (polarIndToLocalMetres(velocity=)); a detector's own store
    is compensated when its scans are added (LoopDetector.add(velocity=), Engine.loop_db_add(velocities=)), not here."""
    keyframes = list(keyframes)
    if len(detector) != len(keyframes):
        raise ValueError(f"closeLoops: the detector holds {len(detector)} scans for {len(keyframes)} keyframes")
    if clouds is None and getattr(detector, "keepClouds", False):      # the detector owns the clouds: keyframe.pointCloud is not read
        edges, table = detector.queryAndVerify(np.arange(len(keyframes), dtype=np.int32), **verify)
        return _optimise(keyframes, edges, table, loopInformation, huber, odomInformation, max_iterations, ctx)
    if clouds is None:
        if rows is None:
            rows = int(np.asarray(keyframes[0].radarPolarImg).shape[0])
        clouds = [polarIndToLocalMetres(k.pointCloud, rows, rangeResolutionM, k.velocity if undistort else None, period) for k in keyframes]
    elif len(clouds) != len(keyframes):
        raise ValueError(f"closeLoops: {len(clouds)} clouds for {len(keyframes)} keyframes")
    idx = np.arange(len(keyframes), dtype=np.int32)
    ci, _, yaw = detector.query(idx)
    edges, table = verifyCandidates(clouds, idx, ci, yaw, **verify)
    return _optimise(keyframes, edges, table, loopInformation, huber, odomInformation, max_iterations, ctx)


def mapFromGraph(detector, graph, **renderMap):
    """The step after closeLoops: the global map of the detector's stored clouds at the graph's poses, graph.get_pose(k) for entry
    k < len(detector) -> Mapping.GlobalMap.  renderMap: LoopDetector.renderMap's keywords (cellM, extent, minHits, minViews, use, grids)"""
    n = len(detector)
    poses = np.array([graph.get_pose(k) for k in range(n)], np.float64).reshape(n, 3)
    return detector.renderMap(poses, **renderMap)


def _optimise(keyframes, edges, table, loopInformation, huber, odomInformation, max_iterations, ctx):
    """closeLoops' second half: the accepted edges into PoseGraphLib.graphFromKeyframes, optimised -> (graph, edges, table)"""
    from . import PoseGraphLib
    loop = [(i, j, z, loopInformation) + ((huber,) if huber is not None else ()) for i, j, z in edges]
    graph = PoseGraphLib.graphFromKeyframes(keyframes, loopEdges=loop, odomInformation=odomInformation, loopInformation=loopInformation, ctx=ctx)
    if edges:
        graph.optimize(max_iterations)
    return graph, edges, table
