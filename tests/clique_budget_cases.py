"""The (case, budget) table of the clique kernel's exhausted node budget (tests/test_clique_budget_cpu.py holds the model to the
oracle and the cases to their conditions; tests/test_gpu_clique_budget.py holds the device to the model).

A case is a correspondence set (prev, new), because the stage entry takes correspondences; its graph is oracle.consistency_graph.
  tie*      the tie-heavy construction of tests/test_gpu_stages.py (static points under a small rigid motion, jitter that straddles
            the threshold, movers) at sizes 20 .. 320, among them 64 / 65 and 128 / 129: from two adjacency words on the degree pass
            is split between the kernel's two wavefronts, from three on unevenly
  big730    the same at 730 correspondences: K * nw > CQ_LDS_ADJ_WORDS = 8192, the adjacency rows are read from global memory
  dense300  300 correspondences, 4 px jitter, 20 % movers, no rotation: phase 1 alone needs more than CQ_MATCH_AFTER = 256 nodes, so
            the matching bound is switched on inside it
  real95, tiny02, tiny08   the reference's real 95-pair fixture and two of tests/golden/clique_lone_sets.npz
The seeds were picked on the CPU, from the model alone, so that the conditions of test_clique_budget_cpu.py hold.
"""
import functools
import os

import numpy as np

import oracle
import clique_budget_model as model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = oracle.DIST_THRESHOLD_PX


def tie_heavy(K, seed, jitter=None, movers=None, rotate=True):
    rng = np.random.default_rng(seed)
    p = rng.uniform(100, 1900, size=(K, 2)).astype(np.float32)
    th = rng.uniform(-0.02, 0.02) if rotate else 0.0
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    n = ((p - 1012) @ R.T + 1012 + rng.uniform(-20, 20, 2)).astype(np.float32)
    n += rng.normal(0, jitter or rng.choice([0.8, 1.6, 2.4]), size=(K, 2)).astype(np.float32)
    mv = rng.permutation(K)[:int(K * (movers or rng.uniform(0.05, 0.4)))]
    n[mv] += rng.normal(0, 12, size=(len(mv), 2)).astype(np.float32)
    return p, n


def _golden(name, tag):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g[tag + "_prev"], g[tag + "_new"]


# name -> a function that returns (prev, new)
CASES = {
    "tie20": lambda: tie_heavy(20, 0),
    "tie41": lambda: tie_heavy(41, 16),
    "tie64": lambda: tie_heavy(64, 5),
    "tie65": lambda: tie_heavy(65, 2),
    "tie100": lambda: tie_heavy(100, 78),
    "tie128": lambda: tie_heavy(128, 7),
    "tie129": lambda: tie_heavy(129, 9),
    "tie200": lambda: tie_heavy(200, 27),
    "tie257": lambda: tie_heavy(257, 3),
    "tie320": lambda: tie_heavy(320, 4),
    "big730": lambda: tie_heavy(730, 0, jitter=1.2, movers=0.25),
    "dense300": lambda: tie_heavy(300, 3, jitter=4.0, movers=0.2, rotate=False),
    "real95": lambda: _golden("outliers", "real95"),
    "tiny02": lambda: _golden("clique_lone_sets", "tiny02"),
    "tiny08": lambda: _golden("clique_lone_sets", "tiny08"),
}
ONE_WAVE_CASES = ("tie65", "tie129", "tie257", "dense300", "tiny02")      # a third of the cases, for the one-wavefront child


def budgets(n1, n2, first):
    """the budgets of a case with phase 1 of n1 nodes, n2 in all, the first non-empty mask at `first`; 0 = the default budget"""
    want = [1, 2, 3, first, n1 - 1, n1, n1 + 1, (n1 + n2) // 2, n2 - 1, n2, n2 + 1]
    return sorted({L for L in want if L >= 1}) + [0]


class Case:
    def __init__(self, name):
        self.name = name
        self.prev, self.new = (np.ascontiguousarray(a, np.float32) for a in CASES[name]())
        self.K = len(self.prev)
        self.adj_words = oracle.consistency_graph(self.prev, self.new, THR)
        self.rows = model.rows_from_words(self.adj_words, self.K)
        self.full = model.run(self.rows, self.K, 0)                     # (mask, n, proven, n1, n2) at the default budget
        self.n1, self.n2 = self.full[3], self.full[4]
        self.first = model.first_nonempty_budget(self.rows, self.K)
        self.budgets = budgets(self.n1, self.n2, self.first)
        self._runs = {0: self.full}

    def run(self, L):
        """the model's (mask, n, proven, n1, n2) at node_limit = L"""
        if L not in self._runs:
            self._runs[L] = model.run(self.rows, self.K, L)
        return self._runs[L]

    def witness(self):
        """phase 1's witness: the mask of every budget n1 <= L < n2 - and, as a plain fact of the model, of L = n1"""
        ctx = model.Ctx(self.rows, self.K, 0)
        return model.solve(ctx, (1 << self.K) - 1, 0, model.NO_TARGET)[1]

    def mask_array(self, L):
        return model.mask_array(self.run(L)[0], self.K)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def all_cases():
    return [case(name) for name in CASES]


# ------------------------------------------------------------------ the engine's lanes
# three synthetic lanes in the (1032, 1020, 1032, 0) layout of gen_inputs.ENGINE_LAYOUTS (sequence seed 4), as tests/test_gpu_engine_flow.py runs them
# (lane 0 forward from the features of frame 0, lane 1 from 40 of them, lane 2 backwards from the features of the last frame), without
# re-detection.  ENGINE_LIMIT was chosen on the CPU - oracle tracker, then the model on each lane-step's correspondence set - so that
# the lane-steps cover every row of the budget table; engine_lane_steps() is that computation and test_clique_budget_cpu.py runs it.
ENGINE_LAYOUT = (1032, 1020, 1032, 0)
ENGINE_SEED = 4
ENGINE_FRAMES = 5
ENGINE_LIMIT = 2


@functools.lru_cache(maxsize=None)
def engine_inputs():
    """-> (records, poses, [(first scan, features)] per lane)"""
    from gen_inputs import layout_sequence
    clip, rows, stride, off = ENGINE_LAYOUT
    recs, poses = layout_sequence(ENGINE_SEED, ENGINE_FRAMES, rows, clip, stride, off, n_movers=12, scintillation=0.3)
    feats = []
    for rec in (recs[0], recs[-1]):
        cart = oracle.convertPolarImageToCartesian(rec[:, off:off + clip].astype(np.float32) / np.float32(255.))
        feats.append(oracle.append_dedupe(np.empty((0, 2)), oracle.getFeatures(cart)[0]).astype(np.float32))
    return recs, poses, [(0, feats[0]), (0, feats[0][:40]), (ENGINE_FRAMES - 1, feats[1])]


def engine_scans(t):
    """the scan of every lane at step t = 1 .. ENGINE_FRAMES - 1"""
    return [t, t, ENGINE_FRAMES - 1 - t]


def regime(n1, n2, L):
    """the row of the budget table: "cut" (L < n1), "witness" (n1 <= L < n2) or "proven" """
    L = L if L > 0 else model.DEFAULT_NODE_LIMIT
    return "cut" if L < n1 else "witness" if L < n2 else "proven"


def reject(prev, new, L):
    """the model's answer for one correspondence set -> (mask bool (K,), n_inliers, proven, regime)"""
    K = len(prev)
    if K == 0:
        return np.zeros(0, bool), 0, True, "proven"
    rows = model.rows_from_words(oracle.consistency_graph(prev, new, THR), K)
    full = model.run(rows, K, 0)
    mask, n, proven, _, _ = model.run(rows, K, L)
    return model.mask_array(mask, K), n, proven, regime(full[3], full[4], L)


@functools.lru_cache(maxsize=None)
def _engine_pyramids():
    clip, rows, stride, off = ENGINE_LAYOUT
    recs = engine_inputs()[0]
    return [oracle.build_pyramid(oracle.convertPolarImageToCartesian(r[:, off:off + clip].astype(np.float32) / 255., want_u8=True)[1], 3)
            for r in recs]


def engine_lane_steps(L):
    """the three lanes on the CPU (oracle tracker, the model's mask at budget L as the lane's next features)
    -> [(step, lane, n_good, n_inliers, proven, regime)]"""
    pyr = _engine_pyramids()
    _, _, starts = engine_inputs()
    scan = [t0 for t0, _ in starts]
    feats = [f for _, f in starts]
    out = []
    for t in range(1, ENGINE_FRAMES):
        for b, s in enumerate(engine_scans(t)):
            nxt, status, err = oracle.klt_on_pyramids(pyr[scan[b]], pyr[s], feats[b])
            good = ((status == 1) & (err < oracle.ERR_THRESHOLD)).flatten()
            mask, n, proven, reg = reject(feats[b][good], nxt[good], L)
            out.append((t, b, int(good.sum()), n, proven, reg))
            feats[b], scan[b] = np.ascontiguousarray(nxt[good][mask], np.float32), s
    return out
