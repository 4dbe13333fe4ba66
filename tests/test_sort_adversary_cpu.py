"""CPU: the rows of tests/sort_adversary_cases.py are what they claim to be - they drive NumPy 1.22.3's argsort into its heapsort
fallback at both levels of the device code (the wavefront's own branch in csrc/npsort_wave.h, the one inside a collected segment in
csrc/blobprune.h), the controls do not, the order of equal heights shows in find_peaks(distance=...)'s peak list, and a fallback
that sorted its segment stably instead would change that list.  Nothing here runs the device code; tests/test_gpu_sort_adversary.py
does, on these rows.

What the trace shows (asserted below):
  killer64_half, killer65_half   no wave-level partition (pr - pl <= 64): one collected segment, a heapsort of 38 / 39 keys inside it
  killer66_half                  the smallest row the wavefront partitions (once); a heapsort of 40 keys inside a collected segment
  killer80_half                  8 wave-level partitions, then a heapsort of 54 keys inside a collected segment
  killer130 .. 2047_half         one wave-level heapsort each: (30, 129), (34, 299), (38, 529), (42, 1023), (42, 2046); half of those
                                 keys are equal in pairs
  organ2047                      6 wave-level segments ((1606, 1865) the longest), 15 inside collected segments, one collected segment
                                 with budget -2; no two equal keys near each other, so its tie order cannot show (a REACHES row)
  organ2047_u8 / _twice / organ1011_u8   1 / 3 / 1 wave-level segments (73 / up to 152 / 69 keys) with equal keys, 17 / 19 / 9 inside
                                 collected segments
The small killer rows (64, 65, 66) give the same peak list under NumPy 1.22's order and under this NumPy's at distances 3, 5 and
10.5, so they are REACHES rows too; 65 and 66 are nevertheless told from a stably sorted fallback (at distance 5 and 3)."""
import numpy as np
import pytest

import peaks_cond_cases as pc
import sort_adversary_cases as sc


@pytest.fixture(scope="module")
def sorted_rows():
    """{name: (KeyRow, the model's permutation, its Trace)}"""
    return {name: (row,) + sc.argsort_keys(row.keys) for name, row in sc.key_rows().items()}


def _ties(row, perm, seg):
    k = row.keys[perm[seg[0]:seg[1] + 1]]
    return len(k) - len(np.unique(k))


def test_thresholds_are_the_headers():
    assert sc.QS_WAVE_MIN == 64 and sc.SMALL_QUICKSORT == 16            # NumPy's SMALL_QUICKSORT; a change needs new rows


def test_model_equals_the_oracle_and_the_host_sort(sorted_rows):
    """two restatements of npy_aquicksort + npy_aheapsort written independently (this Python model, oracle/c/prune.c) and the
    product's host sort (roam_argsort_np122, no GPU needed) give the same permutation, element for element"""
    import oracle
    from radarslampy_amd import getFeatures as gf
    for name, (row, perm, trace) in sorted_rows.items():
        n = len(row.keys)
        assert np.array_equal(np.sort(perm), np.arange(n)), name
        assert np.all(np.diff(row.keys[perm]) >= 0), name
        assert np.array_equal(perm, oracle.argsort_numpy122(row.keys)), name
        assert np.array_equal(perm, oracle.argsort_numpy122(row.f32[1::2])), name         # the heights order like the keys
        assert np.array_equal(perm, gf.argsort_numpy122(row.keys)), name
        if row.u8 is not None:
            assert np.array_equal(perm, oracle.argsort_numpy122(row.u8[1::2])), name


def test_rows_reach_the_fallback_at_both_levels_and_controls_do_not(sorted_rows):
    wave_f32, wave_u8, lane_f32, lane_u8 = [], [], [], []
    whole, resumed, inside = [], [], []
    for name, (row, perm, trace) in sorted_rows.items():
        assert trace.overflow == 0 and trace.most_entries + 2 < sc.WORK_ENTRIES, name      # the work list never fills
        assert all(pr - pl > sc.QS_WAVE_MIN for pl, pr in trace.at(sc.WAVE)), name
        assert all(pr - pl <= sc.QS_WAVE_MIN for pl, pr in trace.at(sc.LANE)), name
        if row.kind == sc.CONTROL:
            assert not trace.heapsorts, (name, trace.heapsorts)
            continue
        assert trace.heapsorts, name
        tied_wave = [s for s in trace.at(sc.WAVE) if _ties(row, perm, s)]
        tied_lane = [s for s in trace.at(sc.LANE) if _ties(row, perm, s)]
        (wave_f32 if row.u8 is None else wave_u8).extend((name, s) for s in tied_wave)
        (lane_f32 if row.u8 is None else lane_u8).extend((name, s) for s in tied_lane)
        lane = set(trace.at(sc.LANE))
        # a collected segment carries its budget and the popped bit to the lane that sorts it: heapsorted as a whole (negative budget,
        # popped), partitioned on with a negative budget (not popped), or with budget left that runs out inside it
        whole += [(name, cd) for pl, pr, cd, popped in trace.collected if cd < 0 and popped and (pl, pr) in lane]
        resumed += [name for pl, pr, cd, popped in trace.collected if cd < 0 and not popped]
        inside += [name for pl, pr, cd, popped in trace.collected if cd >= 0 and any(pl <= a and b <= pr for a, b in lane)]
    assert wave_f32 and wave_u8 and lane_f32 and lane_u8
    assert whole and resumed and inside
    assert any(cd < -1 for _, cd in whole)                  # -2 packs to -3: an arithmetic shift gives -2 back, a division -1
    for m in (130, 300, 530, 1024, 2047):
        row, perm, trace = sorted_rows[f"killer{m}_half"]
        (seg,) = trace.at(sc.WAVE)
        assert seg[1] == m - 1 and _ties(row, perm, seg) > (seg[1] - seg[0]) // 3 and not trace.at(sc.LANE), m
    assert sorted_rows["killer2047_half"][2].at(sc.WAVE) == [(42, 2046)]
    for m, partitions in ((64, 0), (65, 0), (66, 1), (80, 8)):
        trace = sorted_rows[f"killer{m}_half"][2]
        assert len(trace.wave_partitions) == partitions and len(trace.at(sc.LANE)) == 1 and not trace.at(sc.WAVE), m
    organ = sorted_rows["organ2047"][2]
    assert (1606, 1865) in organ.at(sc.WAVE) and len(organ.at(sc.WAVE)) == 6 and len(organ.at(sc.LANE)) == 15
    for name, wave, lane in (("organ2047_u8", 1, 17), ("organ2047_twice", 3, 19), ("organ1011_u8", 1, 9)):
        trace = sorted_rows[name][2]
        assert (len(trace.at(sc.WAVE)), len(trace.at(sc.LANE))) == (wave, lane), name


def test_tie_order_shows_in_the_peak_list(sorted_rows):
    """NumPy 1.22's order against this NumPy's own argsort, through live scipy: without a difference the GPU comparison could not
    tell the orders apart"""
    pytest.importorskip("scipy")
    for name, (row, perm, trace) in sorted_rows.items():
        if row.kind != sc.ADVERSARIAL:
            continue
        img = row.f32[None]
        seen = [d for d in sc.VISIBLE_DISTANCES if not np.array_equal(pc.truth(img, d, None), pc.truth(img, d, None, numpy122=False))]
        assert seen, name


def test_a_stably_sorted_fallback_would_change_the_peak_list(sorted_rows):
    """the bug the GPU test has to see: quicksort as it is, but the heapsorted segments sorted stably, at one level at a time.  The
    truth under the model's permutation is the fixtures' truth (oracle argsort); under the wrong fallback it differs at one of the
    GPU test's distances, on every row listed"""
    pytest.importorskip("scipy")
    expect = {sc.WAVE: [f"killer{m}_half" for m in (130, 300, 530, 1024, 2047)] + ["organ2047_u8", "organ2047_twice", "organ1011_u8"],
              sc.LANE: ["killer65_half", "killer66_half", "killer80_half", "organ2047_u8", "organ2047_twice", "organ1011_u8"]}
    right = {}
    for level, names in expect.items():
        for name in names:
            row, perm, trace = sorted_rows[name]
            img = row.f32[None]
            wrong, wrong_trace = sc.argsort_keys(row.keys, stable_at=(level,))
            assert wrong_trace.heapsorts == trace.heapsorts and np.all(np.diff(row.keys[wrong]) >= 0), (level, name)
            seen = []
            for d in sc.DISTANCES:
                if (name, d) not in right:
                    right[name, d] = sc.truth_with_order(img, d, lambda h: perm)
                    assert np.array_equal(right[name, d], pc.truth(img, d, None)), (name, d)
                if not np.array_equal(right[name, d], sc.truth_with_order(img, d, lambda h: wrong)):
                    seen.append(d)
            assert seen, (level, name)


def test_images_hold_the_rows():
    rows = sc.key_rows()
    imgs = sc.images()
    for name, (kind, names, img) in imgs.items():
        assert img.shape[0] == len(names) and img.shape[1] <= 4096 and img.dtype == (np.float32 if kind == "f32" else np.uint8)
        for i, n in enumerate(names):
            a = getattr(rows[n], kind)
            assert np.array_equal(img[i, :len(a)], a) and not img[i, len(a):].any(), (name, n)
    for k in ("f32", "u8"):
        first, last = imgs[k + "_first"][1], imgs[k + "_last"][1]
        assert rows[first[0]].kind == sc.ADVERSARIAL and rows[first[-1]].kind == sc.CONTROL and last == first[::-1]
    used = {n for kind, names, img in imgs.values() for n in names}
    assert used == set(rows)


def test_sigma_like_keys_never_reach_the_fallback():
    """the sort's other user, adaptiveNMS in retrack_blobs.hip, sorts u8 sigma codes of at most eight distinct values: on 3 000
    random sequences of up to 2048 keys over 2, 3 and 8 values the fallback is never reached, at either level"""
    rng = np.random.default_rng(222)
    for t in range(3000):
        n = int(rng.integers(2, 2049)) if t % 4 == 0 else int(rng.integers(2, 600))
        nv = (2, 3, 8)[t % 3]
        p = rng.dirichlet(np.full(nv, 0.7))
        keys = rng.choice(nv, size=n, p=p).tolist()
        ts, trace = sc.argsort_model(n, lambda i, j: keys[i] < keys[j])
        assert not trace.heapsorts and trace.overflow == 0, (t, n, nv)
