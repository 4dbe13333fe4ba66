"""Crafted clouds and renders for the global map (tests/global_map_model.py): the entries of two cloud-keeping detectors - one at
maxPoints 8192 (BIG, twelve entries), one at maxPoints 64 (SMALL, five entries stored twice, the second time in reverse order) - and
the renders asked of them.  The clouds go in through LoopDetector.addDescriptors(desc, clouds=...); nothing here touches a device."""
import numpy as np

RES = 0.5
SECTORS, RINGS = 7, 3

# the entries of BIG
EMPTY, SINGLE, ONE_CELL, DISTINCT, N8191, N513, N65, N63, TWIN513, EDGES, PAIR_A, PAIR_B = range(12)
PAIR_K = 40                                               # the points of PAIR_A / PAIR_B, six cells apart at RES
GRID_701 = (-87.625, -37.375, 701, 299)                   # at a cell of 0.25 m: N8191's first four points sit in its four corner cells


def big_clouds():
    rng = np.random.default_rng(20)
    box = lambda n: np.stack([rng.uniform(-87.0, 87.0, n), rng.uniform(-37.0, 37.0, n)], axis=1)      # noqa: E731
    one_cell = np.stack([rng.uniform(10.0, 10.5, 8192), rng.uniform(20.0, 20.5, 8192)], axis=1)
    one_cell[:2] = [[10.0, 20.0], [np.nextafter(10.5, 0.0), np.nextafter(20.5, 0.0)]]      # the cell's own corner, and the last doubles inside it
    i, j = np.divmod(np.arange(8192), 64)
    distinct = np.stack([(i - 64 + rng.uniform(0.05, 0.95, 8192)) * RES, (j - 32 + rng.uniform(0.05, 0.95, 8192)) * RES], axis=1)
    n8191 = box(8191)
    n8191[:4] = [[-87.5, -37.25], [87.5, 37.25], [-87.5, 37.25], [87.5, -37.25]]
    n513 = box(513)
    a, b = np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), indexing="ij")
    edges = np.stack([a.ravel() * RES, b.ravel() * RES], axis=1)                # multiples of RES, negative ones and 0 among them
    pi, pj = np.divmod(np.arange(PAIR_K), 8)
    pair = np.stack([3.0 * pi + 0.25, 3.0 * pj + 0.25], axis=1)
    return [np.zeros((0, 2)), np.array([[1.25, -0.75]]), one_cell, distinct, n8191, n513, box(65), box(63), n513.copy(), edges, pair, pair.copy()]


def small_clouds():
    """five clouds of at most 64 points, then the same five in reverse order: entry 9 - e holds the cloud of entry e"""
    rng = np.random.default_rng(21)
    five = [rng.uniform(-30.0, 30.0, (64, 2)), rng.uniform(-30.0, 30.0, (63, 2)), np.zeros((0, 2)), np.array([[-3.0, 4.0]]),
            np.stack([rng.uniform(-2.5, -2.0, 64), rng.uniform(7.0, 7.5, 64)], axis=1)]
    return five + [c.copy() for c in five[::-1]]


def _only(n, *entries):
    use = np.zeros(n, np.int8)
    use[list(entries)] = 1
    return use


def far_poses(n, seed):
    """random headings, +pi and -pi among them, hundreds of metres out"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-300.0, 300.0, n), rng.uniform(-300.0, 300.0, n), rng.uniform(-np.pi, np.pi, n)], axis=1)
    p[0, 2], p[1, 2] = np.pi, -np.pi
    p[min(2, n - 1)] = [-250.5, 199.25, 0.0]
    return p


def big_renders():
    """-> [(name, dict(poses, use, res, extent (None: planned), min_hits, min_views))] on BIG"""
    ident = np.zeros((12, 3))
    twins = far_poses(12, 5)
    twins[TWIN513] = twins[N513]
    out = [("identity, all entries, planned", dict(poses=ident)),
           ("one cell", dict(poses=ident, use=_only(12, ONE_CELL))),
           ("8192 distinct cells", dict(poses=ident, use=_only(12, DISTINCT))),
           ("twins at one far pose", dict(poses=twins, use=_only(12, N513, TWIN513))),
           ("cell edges", dict(poses=ident, use=_only(12, EDGES), extent=(-2.0, -2.0, 8, 8))),
           ("cell edges, cut on four sides", dict(poses=ident, use=_only(12, EDGES), extent=(-1.0, -0.5, 3, 2))),
           ("outside on four sides", dict(poses=ident, use=_only(12, N8191, N513), extent=(-20.0, -10.0, 50, 30))),
           ("far poses, all entries", dict(poses=far_poses(12, 6), res=1.0)),
           ("far poses, a mask", dict(poses=far_poses(12, 7), res=1.0, use=np.array([1, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0], np.int8))),
           ("1 x 1", dict(poses=ident, res=1000.0, extent=(-500.0, -500.0, 1, 1))),
           ("1 x N", dict(poses=ident, res=1.0, extent=(0.0, -60.0, 1, 121))),
           ("N x 1", dict(poses=ident, res=1.0, extent=(-100.0, 0.0, 203, 1))),
           ("701 x 299", dict(poses=ident, res=0.25, extent=GRID_701, use=_only(12, N8191, N63))),
           ("thresholds", dict(poses=ident, min_hits=2, min_views=2)),
           ("min_hits alone", dict(poses=ident, min_hits=3)),
           ("nothing used", dict(poses=ident, use=np.zeros(12, np.int8), extent=(0.0, 0.0, 5, 4)))]
    out += [(f"entry {e} alone", dict(poses=far_poses(12, 8), use=_only(12, e))) for e in (N8191, N513, N65, N63, SINGLE, EMPTY)]
    full = dict(use=None, res=RES, extent=None, min_hits=1, min_views=1)
    return [(name, {**full, **kw}) for name, kw in out]


def small_renders():
    first = np.array([1, 1, 1, 1, 1, 0, 0, 0, 0, 0], np.int8)
    p = far_poses(5, 9)
    poses = np.concatenate([p, p[::-1]])
    full = dict(use=None, res=RES, extent=None, min_hits=1, min_views=1)
    return [(name, {**full, **kw}) for name, kw in
            [("small, all", dict(poses=poses)), ("small, first five", dict(poses=poses, use=first)), ("small, the five again, reversed", dict(poses=poses, use=1 - first)),
             ("small, thresholds", dict(poses=np.zeros((10, 3)), min_hits=2, min_views=2, res=2.0))]]


def expected(clouds, kw, cs):
    """a render of big_renders / small_renders by the model, cs the library's pose table of kw["poses"] -> (extent - the planned one
    where the render names none, as LoopDetector.renderMap plans it -, bounds, the number of points, the model's render)"""
    import global_map_model as model
    b, n = model.bounds(clouds, kw["poses"], cs, kw["use"])
    extent = kw["extent"] or (model.plan(*b, kw["res"]) if n else (0.0, 0.0, 1, 1))
    return extent, b, n, model.render(clouds, kw["poses"], cs, kw["res"], extent, kw["min_hits"], kw["min_views"], kw["use"])


def descriptors(n):
    return np.random.default_rng(1).random((n, SECTORS, RINGS), dtype=np.float32)
