"""CPU: a NumPy model of the walk of the one-sweep integral kernel (csrc/retrack_integral.hip, rt_integral_kernel) - what the kernel's
geometry and schedule rest on, checked without a GPU:
  * the phase builder's rules (retrack_build_phases): a phase = (64-row band, 64-column tile) with one needed bit per 16-row quarter; a
    phase none of whose quarters is needed is left out on a band's left while every column so far is all-zero down to the band's last
    row, and on its right behind the last needed tile;
  * the column direction cut into quarters: per-quarter totals, the base of a quarter = the owner's carry + the totals of the quarters
    above, the owner's carry += the four totals - exact in float64 because a pixel is a multiple of 2^-41 and a column sums to < 2^12;
  * the schedule: between barriers i and i + 1 the column waves run A2(i), A1(i+1) and the row wave B(i-1), C(i-1), on two real tile
    buffers and two tot / cb buffers indexed by the phase's parity - a hazard of the schedule shows as a wrong number.  The row wave
    runs before or after the column waves of its interval: both orders must give the same image.
Needed tiles must equal np.cumsum(np.cumsum(x, 0), 1) bit for bit."""
import numpy as np
import pytest

import oracle

ROWS, Q, WAVES, TILE = 64, 16, 4, 64
SIZES = [132, 300, 336, 384, 496, 1000, 2024, 2048]


def build_phases(need, firstlit, lit, W):
    """need / lit: (quarters, tiles) bool at 16 x 64 granularity; firstlit[c]: first lit row of column c (W: none).
    -> [(band, tile, bits)], in sweep order"""
    H = W
    nbands, ntile = (H + ROWS - 1) // ROWS, (W + TILE - 1) // TILE
    out = []
    for b in range(nbands):
        rend = min(b * ROWS + ROWS - 1, H - 1)
        bits = [sum(int(need[b * WAVES + w, k]) << w for w in range(WAVES)) for k in range(ntile)]
        zero = [bool((firstlit[k * TILE:min(W, (k + 1) * TILE)] > rend).all()) for k in range(ntile)]
        for k in range(ntile):
            skip_l = not bits[k] and all(zero[:k + 1])
            skip_r = not any(bits[k:])
            if skip_l or skip_r:
                assert not lit[b * WAVES:(b + 1) * WAVES, k].any()         # (needed tiles contain every lit pixel)
                continue
            out.append((b, k, bits[k]))
    return out


def walk(x, phases, W, row_wave_first):
    """the kernel's walk over float32 pixels x (W, W): -> the image (NaN where nothing is written)"""
    H = W
    S = np.full((H, W), np.nan)
    tiles = np.full((2, ROWS, TILE), np.nan)
    tot = np.full((2, WAVES, TILE), np.nan)
    cb = np.full((2, TILE), np.nan)
    own = np.zeros((WAVES, 2048 // TILE // WAVES, TILE))                    # a wave's carries: tile group x lane
    v = np.zeros((WAVES, Q, TILE), np.float32)
    vtot = np.zeros((WAVES, TILE))
    nph = len(phases)
    lanes = np.arange(TILE)

    def A1(i, w):
        b, k, _ = phases[i]
        r = b * ROWS + w * Q + np.arange(Q)
        px = x[np.minimum(r, H - 1)[:, None], np.minimum(k * TILE + lanes, W - 1)[None, :]].copy()
        px[r >= H] = 0
        v[w] = px
        s = np.zeros(TILE)
        for q in range(Q):
            s = s + px[q].astype(np.float64)
        vtot[w] = s
        tot[i & 1, w] = s
        if k % WAVES == w:
            cb[i & 1] = own[w, k // WAVES]

    def A2(i, w):
        b, k, _ = phases[i]
        owner = k % WAVES == w
        s, total = cb[i & 1].copy(), vtot[w].copy()
        for q in range(WAVES):
            if q == w or not (q < w or owner):
                continue
            if q < w:
                s = s + tot[i & 1, q]
            total = total + tot[i & 1, q]
        if owner:
            own[w, k // WAVES] += total
        for q in range(Q):
            s = s + v[w, q].astype(np.float64)
            tiles[i & 1, w * Q + q] = s

    def C(i):
        b, k, bits = phases[i]
        for w in range(WAVES):
            r0, c0 = b * ROWS + w * Q, k * TILE
            nr, nc = min(Q, H - r0), min(TILE, W - c0)
            if (bits >> w) & 1 and nr > 0:
                S[r0:r0 + nr, c0:c0 + nc] = tiles[i & 1, w * Q:w * Q + nr, :nc]

    state = dict(carry=np.zeros(ROWS), band=-1)

    def B(i):
        b, k, _ = phases[i]
        if b != state["band"]:
            state["carry"], state["band"] = np.zeros(ROWS), b
        nr, nc = min(ROWS, H - b * ROWS), min(TILE, W - k * TILE)
        t = tiles[i & 1]
        # (np.cumsum along a row is the sequential chain: ((carry + t0) + t1) + ...)
        acc = np.cumsum(np.concatenate([state["carry"][:nr, None], t[:nr, :nc]], axis=1), axis=1)[:, 1:]
        t[:nr, :nc] = acc
        state["carry"][:nr] = acc[:, -1]

    for w in range(WAVES):
        if nph:
            A1(0, w)
    for i in range(nph + 1):                                                # interval i: behind barrier i
        if row_wave_first and i >= 1:
            B(i - 1)
            C(i - 1)
        for w in range(WAVES):
            if i < nph:
                A2(i, w)
            if i + 1 < nph:
                A1(i + 1, w)
        if not row_wave_first and i >= 1:
            B(i - 1)
            C(i - 1)
    return S


_CASE = {}


def _case(W):
    """(pixels float32, the range disc as a pixel mask, NumPy's integral image) of size W, made once"""
    if W not in _CASE:
        if W == 2024:
            from radarslampy_amd import synth
            recs = synth.make_sequence(5, 2, n_static=460, n_movers=24, distortion=True)[0]
            pay = np.ascontiguousarray(recs[0][:, 11:11 + 2025])
        else:
            pay = np.random.default_rng(W).integers(0, 256, (400, W), dtype=np.uint8)
        x = oracle.convertPolarImageToCartesian(pay.astype(np.float32) / np.float32(255.))
        disc = oracle.convertPolarImageToCartesian(np.ones(pay.shape, np.float32)) > 0
        assert x.shape == (W, W) and not x[~disc].any()
        x64 = x.astype(np.float64)
        _CASE[W] = (x, disc, np.cumsum(np.cumsum(x64, 0), 1))
    return _CASE[W]


def _tiles_of(mask, W):
    nq, nt = WAVES * ((W + ROWS - 1) // ROWS), (W + TILE - 1) // TILE
    pad = np.zeros((nq * Q, nt * TILE), bool)
    pad[:W, :W] = mask
    return pad.reshape(nq, Q, nt, TILE).any(axis=(1, 3))


def _dilate(t):
    p = np.pad(t, 1)
    return np.logical_or.reduce([p[1 + dr:p.shape[0] - 1 + dr, 1 + dc:p.shape[1] - 1 + dc] for dr in (-1, 0, 1) for dc in (-1, 0, 1)])


@pytest.mark.parametrize("superset", [False, True], ids=["need_dilated", "need_random_superset"])
@pytest.mark.parametrize("W", SIZES)
def test_walk_equals_numpy_on_needed_tiles(W, superset):
    x, disc, want = _case(W)
    # the premise of the quarters: every partial column sum is exact
    assert not np.mod(x.astype(np.float64) * 2.0 ** 41, 1.0).any()
    assert np.cumsum(x.astype(np.float64), 0)[-1].max() < 2.0 ** 12
    lit = _tiles_of(disc, W)
    need = _dilate(lit)
    nq_live = (W + Q - 1) // Q
    need[nq_live:] = False                                                  # (quarters below the image: no determinant block there)
    if superset:
        need |= np.random.default_rng(W + 1).random(need.shape) < 0.3
        need[nq_live:] = False
    firstlit = np.where(disc.any(0), disc.argmax(0), W)
    phases = build_phases(need, firstlit, lit, W)
    listed = {(b, k) for b, k, _ in phases}
    ntile = (W + TILE - 1) // TILE
    # every needed quarter is in the list with its bit; what is left out holds zero pixels only
    for qr, k in np.argwhere(need):
        assert (qr // WAVES, int(k)) in listed
    for b in range((W + ROWS - 1) // ROWS):
        for k in range(ntile):
            if (b, k) not in listed:
                assert not x[b * ROWS:(b + 1) * ROWS, k * TILE:(k + 1) * TILE].any(), (b, k)
    assert [(b, k) for b, k, _ in phases] == sorted(listed)                 # sweep order: band-major, tiles ascending
    written = np.kron(need, np.ones((Q, TILE), bool))[:W, :W]
    images = [walk(x, phases, W, first) for first in (False, True)]
    for S in images:
        assert np.array_equal(np.isnan(S), ~written)                        # exactly the needed 16 x 64 tiles are written
        assert np.array_equal(S[written], want[written])                    # ... with NumPy's bits
