"""PoseGraphLib.PoseGraphOptimization (PoseGraphLib.py:5-43) on the device: the reference's g2o wrapper - add_vertex, add_edge,
optimize, get_pose - over roam_pose_graph_optimize (csrc/posegraph.hip).  The project is 2-D throughout, so vertices and
measurements are SE(2) poses (x, y, theta) where the reference's wrapper says SE3; the error, the Jacobians and the update are g2o's
EdgeSE2 / VertexSE2 and the minimiser its OptimizationAlgorithmLevenberg (include/roam_abi.h states them; PARITY UNPINNED against g2o,
docs/PARITY.md).  BundleAdjustment (PoseGraphLib.py:46-98) is camera-model specific and has no counterpart.

Cost: there is no vertex reordering.  Vertices are numbered in insertion order and block row k of the system is stored from the
lowest-numbered neighbour of vertex k to the diagonal, so a graph costs its envelope - about the vertex count plus the sum of j - i
over its non-consecutive edges (_ffi.pose_graph_plan gives the figure).  Insert vertices along the trajectory."""
import numpy as np

from . import _ffi
from .utils import convertTransformToPose, normalize_angles


def _pose3(p, what):
    p = np.array(p, np.float64)
    if p.shape == (3, 3):
        p = convertTransformToPose(p)
    if p.shape != (3,):
        raise ValueError(f"{what}: (3,) [x, y, theta] or a 3 x 3 transform, not {p.shape}")
    return p


class PoseGraphOptimization():
    def __init__(self, ctx=None):
        self.ctx = ctx
        self._index = {}                    # id -> vertex number, in insertion order
        self._poses, self._fixed = [], []
        self._ij, self._meas, self._info, self._huber = [], [], [], []
        self.stats = None

    def add_vertex(self, id, pose, fixed=False):
        if id in self._index:
            raise ValueError(f"add_vertex: vertex {id!r} is already in the graph")
        self._index[id] = len(self._poses)
        self._poses.append(_pose3(pose, "add_vertex"))
        self._fixed.append(bool(fixed))

    def add_edge(self, vertices, measurement, information=np.eye(3), robust_kernel=None):
        """vertices: a pair of ids (from, to); measurement: from^-1 to; robust_kernel: None or a Huber width"""
        a, b = vertices
        for v in (a, b):
            if v not in self._index:
                raise ValueError(f"add_edge: no vertex {v!r}")
        info = np.array(information, np.float64)         # a copy: the caller's matrix (and the shared default) may change later
        if info.shape != (3, 3):
            raise ValueError(f"add_edge: information 3 x 3, not {info.shape}")
        self._ij.append((self._index[a], self._index[b]))
        self._meas.append(_pose3(measurement, "add_edge"))
        self._info.append(info)
        self._huber.append(0.0 if robust_kernel is None else float(robust_kernel))

    def graph(self):
        """the graph as Context.pose_graph_optimize takes it"""
        E = len(self._ij)
        return (np.array(self._poses, np.float64).reshape(-1, 3), np.array(self._fixed, bool), np.array(self._ij, np.int32).reshape(E, 2),
                np.array(self._meas, np.float64).reshape(E, 3), np.array(self._info, np.float64).reshape(E, 3, 3),
                np.array(self._huber, np.float64) if any(self._huber) else None)

    def optimize(self, max_iterations=20):
        optimizeGraphs([self], max_iterations)

    def get_pose(self, id):
        return np.array(self._poses[self._index[id]])


def optimizeGraphs(graphs, max_iterations=20):
    """optimize() of several PoseGraphOptimization objects in one device call; each gets its poses and its .stats"""
    graphs = list(graphs)
    ctx = next((g.ctx for g in graphs if g.ctx is not None), None) or _ffi.default_context()
    poses, stats = ctx.pose_graph_optimize([g.graph() for g in graphs], max_iterations=max_iterations)
    for g, p, s in zip(graphs, poses, stats):
        g._poses = [row for row in p]
        g.stats = s


def odometryEdges(poses):
    """the N - 1 relative measurements x_k^-1 x_{k+1} of a pose list (N, 3) -> (N - 1, 3)"""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    c, s = np.cos(p[:-1, 2]), np.sin(p[:-1, 2])
    dx, dy = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, normalize_angles(p[1:, 2] - p[:-1, 2])], axis=1)


def graphFromKeyframes(keyframes, loopEdges=(), odomInformation=np.eye(3), loopInformation=np.eye(3), ctx=None):
    """A pose graph over keyframes - anything with .pose, as Mapping.DeviceMap(eng, lane).keyframes and Map.keyframes return:
    vertex k = keyframe k (the first one fixed), odometry edges between consecutive keyframes measured from their poses, and
    loopEdges = (i, j, measurement[, information[, huber]]) tuples between keyframe numbers."""
    g = PoseGraphOptimization(ctx)
    poses = np.array([np.asarray(k.pose, np.float64).reshape(3) for k in keyframes]).reshape(-1, 3)
    for k, p in enumerate(poses):
        g.add_vertex(k, p, fixed=(k == 0))
    for k, z in enumerate(odometryEdges(poses)):
        g.add_edge((k, k + 1), z, odomInformation)
    for e in loopEdges:
        i, j, z = e[:3]
        g.add_edge((i, j), z, e[3] if len(e) > 3 else loopInformation, e[4] if len(e) > 4 else None)
    return g
