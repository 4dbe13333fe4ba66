"""CPU (-m "not gpu"): the scan-context contract without a device.  roam_scan_context_plan (host code of libroam_hip.so) returns the
model's bin edges and refuses every bad argument; the Python wrappers raise ValueError before a device is needed; the model
(tests/scan_context_model.py) equals an independent loop-by-loop evaluation and gives the known answer on rolled images; the
tolerance of the GPU test is measured here (ten times the largest difference between the model's summation order and the kernel's,
both float64) and the conditions that keep the GPU test's discrete comparisons honest are asserted on the model alone: the shifts
are decided on at least 95 % of the pairs of every case, and the ranks of every top-k case are separated by more than twice the
tolerance.  On the project's synthetic world the model ranks every revisit's true place first at no more than half the next
place's distance, at floor 0 and floor 30, with the yaw within one sector."""
import ctypes as C

import numpy as np
import pytest

import scan_context_cases as cases
import scan_context_model as model
from radarslampy_amd import _ffi


@pytest.mark.parametrize("name", list(cases.DESCRIBE_CASES))
def test_plan_returns_the_models_edges(name):
    S, R, clip_px = cases.DESCRIBE_CASES[name]
    _, rows, cols = cases.describe_images(name).shape
    clip, re, ce = _ffi.scan_context_plan(rows, cols, clip_px, S, R)
    want_re, want_ce = model.bin_edges(rows, cols, clip_px, S, R)
    assert clip == model.clip_of(cols, clip_px) and np.array_equal(re, want_re) and np.array_equal(ce, want_ce)
    assert np.all(np.diff(re) >= 1) and np.all(np.diff(ce) >= 1) and re[-1] == rows and ce[-1] == clip


def test_plan_edges_400_rows_60_sectors():
    _, re, _ = _ffi.scan_context_plan(400, 2025, None, 60, 20)
    assert set(np.diff(re)) == {6, 7}


BAD_PLANS = [(400, 2025, 0, 1, 20), (400, 2025, 0, 257, 20), (400, 2025, 0, 60, 0), (400, 2025, 0, 60, 129), (59, 2025, 0, 60, 20),
             (65537, 2025, 0, 60, 20), (400, 0, 0, 60, 20), (400, 2025, 19, 60, 20), (400, 19, 0, 60, 20), (400, 5000, 0, 60, 20),
             (400, 5000, 4097, 60, 20)]


@pytest.mark.parametrize("args", BAD_PLANS)
def test_plan_refuses(args):
    lib = _ffi.load_library()
    re, ce = np.zeros(300, np.int32), np.zeros(200, np.int32)
    assert lib.roam_scan_context_plan(*args, _ffi._ptr(re), _ffi._ptr(ce)) == _ffi.ROAM_E_ARG
    rows, cols, clip_px, S, R = args
    with pytest.raises(ValueError):
        _ffi.scan_context_plan(rows, cols, clip_px, S, R)


def test_plan_accepts_the_limits_and_null_outputs():
    lib = _ffi.load_library()
    assert lib.roam_scan_context_plan(65536, 5000, 4096, 256, 128, None, None) == _ffi.ROAM_OK
    assert lib.roam_scan_context_plan(2, 1, 0, 2, 1, None, None) == _ffi.ROAM_OK


def test_null_context_is_rejected():
    lib = _ffi.load_library()
    n = C.c_int32(0)
    assert lib.roam_scan_context_f32(None, None, 1, 8, 8, 8, 64, 0, 2, 1, 0.0, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_create(None, 1, 60, 20, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_destroy(None, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_count(None, C.byref(n)) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_add_f32(None, None, None, 1, 8, 8, 8, 64, 0, 0.0, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_add_desc(None, None, None, 1, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_get(None, None, 0, 1, None) == _ffi.ROAM_E_ARG
    assert lib.roam_engine_loop_db_add(None, None, 1, None, 0, 0, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_query(None, None, 1, None, None, 1, 0.0, None, None, None, None, None) == _ffi.ROAM_E_ARG


def test_python_wrappers_raise_value_error_without_a_device():
    from radarslampy_amd import LoopClosure as lc
    img = np.zeros((64, 128), np.float32)
    for kw in (dict(sectors=1), dict(sectors=257), dict(rings=0), dict(rings=129), dict(sectors=65), dict(rings=20, clip_px=19),
               dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(sectors=16.0), dict(clip_px=2.5)):
        with pytest.raises(ValueError):
            lc.scanContext(img, **{**dict(sectors=16, rings=8), **kw})
    with pytest.raises(ValueError):
        lc.scanContext(np.zeros(5, np.float32))
    with pytest.raises(ValueError):
        lc.scanContext(np.zeros((64, 5000), np.float32), 16, 8)                 # clip above ROAM_SCAN_CONTEXT_MAX_CLIP
    with pytest.raises(ValueError):
        lc.scanContextDistance(np.zeros((16, 8), np.float32), np.zeros((16, 9), np.float32))
    for kw in (dict(capacity=0), dict(sectors=1), dict(rings=129), dict(floor=-0.5), dict(min_gap=0), dict(k=0), dict(k=33),
               dict(max_distance=float("nan")), dict(capacity=10 ** 9), dict(clip_px=-3)):
        with pytest.raises(ValueError):
            lc.LoopDetector(**{**dict(capacity=8), **kw})
    with pytest.raises(ValueError):
        _ffi.loop_query_args(5, [5], [0], 1, 0.2)
    with pytest.raises(ValueError):
        _ffi.loop_query_args(5, [0, 1], [0], 1, 0.2)
    with pytest.raises(ValueError):
        _ffi.loop_query_args(5, [], [], 1, 0.2)


def test_model_equals_the_loop_by_loop_evaluation():
    rng = np.random.default_rng(3)
    worst = 0.0
    for S, R in ((7, 3), (2, 1), (12, 5), (16, 8)):
        D = rng.random((6, S, R), dtype=np.float32)
        D[1, : S // 2] = 0
        D[2] = 0
        D[3] = D[3, 0]
        for i in range(6):
            dk = model.shift_distances(D[i], D)
            for j in range(6):
                d, k, all_k = model.distance_brute(D[i], D[j])
                worst = max(worst, float(np.abs(dk[j] - np.array(all_k)).max()))
                assert np.abs(dk[j] - np.array(all_k)).max() <= 1e-14
                md, mk = model.distance(D[i], D[j])
                assert abs(md - d) <= 1e-14 and (mk == k or abs(all_k[mk] - d) <= 1e-14)
        assert model.distance(D[0], D[2]) == (1.0, 0) and model.distance(D[2], D[0]) == (1.0, 0)      # all-zero: 1 and shift 0
        assert model.distance(D[0], D[3])[1] == 0                                                     # sector-constant candidate: a tie
    print(f"model against the loop-by-loop evaluation: largest |d_k difference| {worst:.3g}")


def test_rolled_image_gives_a_rolled_descriptor_and_its_shift():
    """rows a multiple of S: a roll by whole sectors is a roll of the descriptor, bit for bit"""
    rng = np.random.default_rng(4)
    S, R, per = 20, 6, 3
    img = rng.random((S * per, 90), dtype=np.float32)
    codes = rng.integers(0, 256, (S * per, 90)).astype(np.uint8)
    d0, c0 = model.describe_f32(img, S, R, None, 0.1), model.describe_u8(codes, S, R, 80, 30)
    tol = cases.tolerance()
    for sh in (1, 7, 19):
        assert np.array_equal(model.describe_f32(np.roll(img, sh * per, axis=0), S, R, None, 0.1), np.roll(d0, sh, axis=0))
        assert np.array_equal(model.describe_u8(np.roll(codes, sh * per, axis=0), S, R, 80, 30), np.roll(c0, sh, axis=0))
        # the rolled scan is the candidate: c[(s + sh) mod S] = q[s], so the minimum is at shift sh; as the query the shift is S - sh
        d, k = model.distance(d0, np.roll(d0, sh, axis=0))
        assert d <= tol and k == sh, (sh, d, k)
        d, k = model.distance(np.roll(d0, sh, axis=0), d0)
        assert d <= tol and k == S - sh, (sh, d, k)


def test_u8_and_f32_forms_agree_on_codes():
    """the float32 form on codes / 255 is the integer form up to the rounding of the float32 image values"""
    codes = cases.real_codes()[0]
    a = model.describe_u8(codes, 60, 20, 2025, 0)
    b = model.describe_f32(codes.astype(np.float32) / np.float32(255.0), 60, 20, 2025, 0.0)
    assert np.abs(a.astype(np.float64) - b).max() <= 2e-7 * a.max()


def test_tolerance_and_shift_condition():
    tol = cases.tolerance()
    for name, v in cases.tolerance_measured().items():
        print(f"{name}: model order against kernel order, largest |d_k difference| {v:.3g}")
    print(f"tolerance = 10 x the largest = {tol:.3g}")
    assert 0 < tol < 1e-9          # float64 arithmetic: anything larger means one of the two orders is wrong
    for name in cases.DISTANCE_CASES:
        dec = cases.decided(name)
        print(f"{name}: shift decided on {dec.sum()} of {dec.size} pairs ({100.0 * dec.mean():.2f} %)")
        assert dec.mean() >= 0.95, name


def test_degenerate_entries_in_the_model():
    for name, (S, R, n, _, _) in cases.DISTANCE_CASES.items():
        if n < 8:
            continue
        D, q = cases.distance_case(name)
        dist, shift, _ = cases.distance_model(name)
        assert np.all(dist[:, cases.ALL_ZERO] == 1.0) and np.all(shift[:, cases.ALL_ZERO] == 0)
        assert np.all(shift[:, cases.SECTOR_CONSTANT] == 0)
        a, b, c = cases.triple(n)
        assert np.array_equal(dist[:, a], dist[:, b]) and np.array_equal(dist[:, a], dist[:, c])


def test_topk_conditions():
    """on every top-k case the model's distances under the threshold, the boundary at rank k and the boundary at max_distance are
    separated by more than twice the tolerance; the planted entries are exactly what the threshold admits, in planting order"""
    tol = cases.tolerance()
    D, q, slots, shifts = cases.topk_case()
    dist, shift, _ = cases.topk_model()
    gaps = []
    for tag, max_index, k, max_distance in cases.topk_queries():
        for i in range(len(q)):
            d = np.sort(dist[i, :max_index[i]])
            under = d[d <= max_distance]
            assert np.all(np.diff(under) > 2 * tol), tag                          # consecutive ranks, the boundary at rank k included
            gaps += list(np.diff(under[:k + 1]))
            if np.isfinite(max_distance):
                assert np.all(np.abs(d - max_distance) > 2 * tol), tag
    for i in range(len(q)):
        d = dist[i, :len(D) - cases.TOPK_QUERIES]
        admitted = np.flatnonzero(d <= cases.TOPK_MAX_DISTANCE)
        assert np.array_equal(admitted[np.argsort(d[admitted])], slots[i]), (i, admitted, slots[i])
        assert np.array_equal(shift[i, slots[i]], shifts[i])
        others = np.delete(d, slots[i])
        print(f"top-k query {i}: planted at {np.round(d[slots[i]], 4)}, the nearest other entry at {others.min():.4f}")
        assert others.min() > cases.TOPK_MAX_DISTANCE + 2 * tol
    print(f"smallest gap between consecutive ranks {min(gaps):.3g}")
    ci, cd, cs = model.candidates(dist, shift, np.full(3, len(D) - 3), cases.TOPK_MAX_DISTANCE, 32)
    assert np.array_equal(ci[:, :8], slots) and np.all(ci[:, 8:] == -1) and np.all(np.isinf(cd[:, 8:])) and np.all(cs[:, 8:] == 0)


@pytest.mark.parametrize("floor_code", cases.REVISIT_FLOOR_CODES)
def test_revisit_world_in_the_model(floor_code):
    D = cases.revisit_descriptors(floor_code)
    n_places = len(cases.PLACES)
    dist, shift, _ = model.distances(D[n_places:], D[:n_places])
    for t, (place, _) in enumerate(cases.REVISITS):
        order = np.argsort(dist[t])
        ratio = dist[t, order[0]] / dist[t, order[1]]
        true = cases.revisit_true_shift(t)
        off = abs((shift[t, place] - true + 30) % 60 - 30)
        print(f"floor {floor_code}, revisit {t}: place {order[0]} at {dist[t, order[0]]:.4f}, next {order[1]} at {dist[t, order[1]]:.4f} "
              f"(ratio {ratio:.2f}); shift {shift[t, place]}, true {true:.2f} sectors")
        assert order[0] == place and ratio <= 0.5 and off <= 1.0
