"""GPU (-m gpu): the device blob bookkeeping (csrc/retrack_blobs.hip: candidate order, cKDTree build and query_pairs order, CPython
set order, _prune_blobs, NumPy-1.22 argsort, SSC) alone, through roam_engine_debug_blobs, on the crafted candidate lists of
tests/blob_book_cases.py - tests/test_blob_book_cpu.py holds every case to the branch it names.  Everything is exact: kp rows, kp_n,
sel, sel_n and the flags against the CPU truth (blob_book_cases.truth), and the device's candidate pairs against the oracle's in
query_pairs' EMISSION ORDER (the slid-split bound of slid_flip_20_20 shows there and nowhere else), no tolerance anywhere.

Two engines shared by the module: three lanes at W = 2048 (every case alone - rt_book_kernel - and the overflow cases between
neighbours) and 512 lanes at W = 132 (rows 64, clip 132) for the batch forms: P = 256 (emit + small + full class kernels) and P = 512
(longest list first), filled with three cheap cases of different lengths, the hard cases first, in the middle and last.

Device figures: not yet recorded."""
import numpy as np
import pytest

import blob_book_cases as K

pytestmark = pytest.mark.gpu

W_BIG, W_SMALL = 2048, 132
CASES = K.cases()
SMALL = [c for c in CASES if c.side <= K.SMALL_SIDE]
FILL = ("count_17", "count_100", "count_2")
_truth, _pairs = {}, {}


def _scans(clip, rows, n=2):
    """random payloads with bright squares (tests/test_gpu_retrack.py): 1412 and 1173 determinant maxima, 27 057 and 23 299 candidate
    pairs - the full class with its set tables in global memory, and inside every capacity (beyond 2048 candidates the kept subset is
    arbitrary, beyond 32 767 pairs the result is not the reference's)"""
    rng = np.random.default_rng(140)
    out = []
    for _ in range(n):
        pay = (rng.random((rows, clip)) * 3).astype(np.uint8)
        for _ in range(60):
            a, r = int(rng.integers(0, rows)), int(rng.integers(200, clip - 5))
            pay[max(0, a - 2):a + 2, max(0, r - 2):r + 2] = rng.integers(150, 255)
        out.append(pay)
    return out


def _engine(lanes, clip, rows):
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    ctx = _ffi.Context(0)
    eng = Engine(lanes, 2, ctx=ctx, rows=rows, stride=clip, payload_off=0, clip=clip, retrack_on_device=True, retrack_slots=1)
    return ctx, eng


@pytest.fixture(scope="module")
def big():
    ctx, eng = _engine(3, W_BIG, 400)
    yield eng
    eng.close()
    ctx.close()


@pytest.fixture(scope="module")
def small():
    ctx, eng = _engine(512, W_SMALL, 64)
    yield eng
    eng.close()
    ctx.close()


def truth(c, W):
    if (c.name, W) not in _truth:
        _truth[(c.name, W)] = K.truth(c.rc, c.val, W)
    return _truth[(c.name, W)]


def emission(c):
    """the candidate pairs i << 16 | j in the order live-scipy-checked oracle.ckdtree_pairs emits them; as many as the device keeps
    (none after a tree / task overflow: its pair scratch then holds the traversal's lists)"""
    if c.name not in _pairs:
        import oracle
        b = K.blobs_of(c.rc, c.val)
        p = oracle.ckdtree_pairs(b[:, :2], K.radius(K.unpack(c.rc)[2]))[0] if len(b) > 1 and not K.flags_of(c) & K.F_TREE else np.empty((0, 2), np.int64)
        _pairs[c.name] = ((p[:, 0] << 16) | p[:, 1]).astype(np.uint32)[:K.MAX_PAIRS]
    return _pairs[c.name]


def run(eng, cases):
    """the cases as ONE call of P = len(cases) problems -> per problem dict(kp_n, kp, flags, sel_n, sel, pairs = the device's pair list
    cut to the length of emission())"""
    rows = max(len(c.rc) for c in cases)
    rc = np.zeros((len(cases), rows), np.uint32)
    val = np.zeros((len(cases), rows), np.float64)
    for p, c in enumerate(cases):
        rc[p, :len(c.rc)] = c.rc
        val[p, :len(c.rc)] = c.val
    out = eng.debug_blobs(rc, val, [c.cand_n or len(c.rc) for c in cases], want_pairs=True)
    res = [{k: v[p] for k, v in out.items()} for p in range(len(cases))]
    for o, c in zip(res, cases):
        o["pairs"] = o["pairs"][:len(emission(c))].copy()
    return res


def check_truth(o, c, W):
    kp, sel = truth(c, W)
    assert o["flags"] == K.flags_of(c), (c.name, o["flags"])
    assert o["kp_n"] == len(kp), (c.name, o["kp_n"], len(kp))
    assert np.array_equal(o["kp"][:len(kp)], kp), c.name
    assert np.isnan(o["kp"][len(kp):]).all(), c.name                          # rows beyond kp_n: never written
    assert o["sel_n"] == len(sel), (c.name, o["sel_n"], len(sel))
    assert np.array_equal(o["sel"][:len(sel)], sel), c.name
    assert np.array_equal(o["pairs"], emission(c)), c.name                     # query_pairs' emission order


def check_sane(o, c, W):
    """an overflow case: the documented flag alone, every output finite and in range"""
    n = min(len(c.rc), K.MAX_PTS)
    assert o["flags"] == K.flags_of(c), (c.name, o["flags"])
    assert np.array_equal(o["pairs"], emission(c)), c.name                     # the first 32767 pairs of a pair overflow: still in order
    assert 0 <= o["kp_n"] <= n and 0 <= o["sel_n"] <= o["kp_n"], (c.name, o["kp_n"], o["sel_n"])
    kp = o["kp"][:o["kp_n"]]
    assert np.isfinite(kp).all() and (kp[:, :2] >= 0).all() and (kp[:, :2] < W).all() and np.isin(kp[:, 2], K.SIG[1:]).all(), c.name
    have = {tuple(r) for r in K.blobs_of(c.rc, c.val).tolist()}
    assert all(tuple(r) in have for r in kp.tolist()) and len({tuple(r) for r in kp.tolist()}) == len(kp), c.name
    sel = o["sel"][:o["sel_n"]]
    assert (sel >= 0).all() and (sel < max(o["kp_n"], 1)).all() and len(set(sel.tolist())) == len(sel), c.name


def same(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in ("kp_n", "kp", "flags", "sel_n", "pairs")) and \
        np.array_equal(x["sel"][:max(x["sel_n"], 0)], y["sel"][:max(y["sel_n"], 0)])


# ------------------------------------------------------------------------------------------------ every case alone: rt_book_kernel
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_alone_equals_the_truth(big, c):
    o = run(big, [c])[0]
    print(c.name, "kp_n", o["kp_n"], "sel_n", o["sel_n"], "flags", o["flags"])
    if K.flags_of(c) & (K.F_TREE | K.F_PAIR):
        check_sane(o, c, W_BIG)
    else:
        check_truth(o, c, W_BIG)


def test_rows_in_any_order_give_the_same_result(big):
    """K4 ranks the rows by key: the order the determinant kernel appended them in does not matter"""
    rng = np.random.default_rng(1)
    for name in ("pairs_4915", "ties_four_responses", "ties_both_layers", "slid_flip_20_20"):
        c = K.by_name(name)
        base = run(big, [c])[0]
        o = np.argsort(c.rc)
        for p in (o, o[::-1], rng.permutation(len(o))):
            assert same(run(big, [c._replace(rc=c.rc[p], val=c.val[p])])[0], base), name


# ------------------------------------------------------------------------------------------------ the batch forms
@pytest.fixture(scope="module")
def lone_small(small):
    """every small-image case alone on the small engine, held to the truth (SSC on 132 x 132) - the batch results must equal these"""
    out = {}
    for c in SMALL:
        o = run(small, [c])[0]
        (check_sane if K.flags_of(c) & (K.F_TREE | K.F_PAIR) else check_truth)(o, c, W_SMALL)
        out[c.name] = o
    return out


@pytest.mark.parametrize("P", [255, 256, 512])
def test_batch_forms_equal_the_lone_runs(small, lone_small, P):
    """255: the largest one-kernel launch; 256: emit + small class + full class + SSC kernels; 512: the same behind blob_order (the lists
    have 2 .. 2048 rows, so the order really permutes)"""
    hard = [c for c in SMALL if c.name not in FILL]
    first, mid, last = K.by_name("pairs_4915"), K.by_name("dense_field"), K.by_name("overflow_tasks")
    rest = [c for c in hard if c.name not in (first.name, mid.name, last.name)]
    batch = [K.by_name(FILL[p % 3]) for p in range(P)]
    batch[0], batch[P // 2], batch[P - 1] = first, mid, last
    free = [p for p in range(1, P - 1) if p != P // 2]
    for k, c in enumerate(rest):                                              # the others spread over the batch
        batch[free[k * (len(free) // len(rest))]] = c
    assert {c.name for c in batch} >= {c.name for c in hard} and len({len(c.rc) for c in batch}) > 8
    got = run(small, batch)
    for p, c in enumerate(batch):
        assert same(got[p], lone_small[c.name]), (P, p, c.name)


# ------------------------------------------------------------------------------------------------ overflow between neighbours
@pytest.mark.parametrize("name", ["overflow_pairs", "overflow_tasks", "overflow_cand"])
def test_overflow_raises_its_flag_and_leaves_the_neighbours_alone(big, name):
    a, c, b = K.by_name("count_100"), K.by_name(name), K.by_name("pairs_1229")
    la, lb = run(big, [a])[0], run(big, [b])[0]
    got = run(big, [a, c, b])
    assert same(got[0], la) and same(got[2], lb)
    check_truth(got[0], a, W_BIG)
    check_truth(got[2], b, W_BIG)
    if name == "overflow_cand":
        check_truth(got[1], c, W_BIG)                                         # the truth on the 2048 rows given, flag 1
    else:
        check_sane(got[1], c, W_BIG)


# ------------------------------------------------------------------------------------------------ arguments and engine state
def test_bad_arguments_are_refused(small):
    from radarslampy_amd import _ffi
    ok = K.by_name("count_17")
    r, c, l = K.unpack(ok.rc)

    def refused(rc, val, cand_n=None):
        with pytest.raises(_ffi.RoamError) as e:
            small.debug_blobs(rc, val, cand_n)
        assert e.value.code == _ffi.ROAM_E_ARG

    refused(np.zeros((0, 17), np.uint32), np.zeros((0, 17)))                                      # P = 0
    refused(np.tile(ok.rc, (513, 1)), np.tile(ok.val, (513, 1)))                                  # P > lanes
    for bad in (K.pack([W_SMALL], [5], [1]), K.pack([5], [W_SMALL], [2]), K.pack([5], [5], [0]), K.pack([5], [5], [3]), ok.rc[:1]):
        rc = np.concatenate([ok.rc, bad])[None]                                                   # row / col >= W, layer 0 / 3, a repeated key
        refused(rc, np.zeros(rc.shape))
    refused(ok.rc[None], ok.val[None], [18])                                                      # more candidates than rows, within 2048
    refused(ok.rc[None], ok.val[None], [-1])
    assert same(run(small, [ok])[0], run(small, [ok])[0])                                         # and the engine still works


def test_a_step_after_the_call_equals_a_twin_engine(big):
    """the scratch is left as a detection expects it: first detections and a step on the engine that ran the hardest cases (all three
    overflows last) give the records of an engine that never did, byte for byte"""
    ctx2, twin = _engine(3, W_BIG, 400)
    scans = _scans(W_BIG, 400)
    run(big, [K.by_name("overflow_cand"), K.by_name("overflow_pairs"), K.by_name("overflow_tasks")])
    feats = []
    for eng in (big, twin):
        for t, s in enumerate(scans):
            eng.upload_scan(t, s)
        eng.init_lanes_detect(0, [0, 1, 0], np.zeros((3, 3)))
        f0 = [eng.lane_features(b) for b in range(3)]
        eng.set_features(1, f0[1][:20])                                        # lane 1 re-detects in the step
        eng.step([1, 0, 1])
        feats.append((f0, eng.results_array().tobytes(), [eng.lane_features(b) for b in range(3)]))
    twin.close()
    ctx2.close()
    (a0, ra, a1), (b0, rb, b1) = feats
    assert all(len(f) > 100 for f in a0)
    assert all(np.array_equal(x, y) for x, y in zip(a0, b0)) and ra == rb and all(np.array_equal(x, y) for x, y in zip(a1, b1))
    res = np.frombuffer(ra, dtype=big.results_array().dtype)
    assert res["n_after_retrack"][1] > 100 and not ((res["flags"] >> 8) & 0xf).any()      # the step did run the device detection, no overflow
    import oracle
    cart = oracle.convertPolarImageToCartesian(scans[0].astype(np.float32) / np.float32(255.))
    assert np.array_equal(a0[0], oracle.append_dedupe(np.empty((0, 2)), oracle.getFeatures(cart)[0]))
