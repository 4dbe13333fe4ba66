"""NumPy float64 model of the screen in sd_tile_fast (csrc/retrack_det.hip): the six boxes the fast path always reads (per box size
yy-mid, yy-side, xx-mid), the bound that decides whether the xx-side box is read, and its margin - every operation in the kernel's
order, each rounded once (NumPy float64 arithmetic does not contract).  It also restates the screen the other way round (dxx exact,
the yy-side box conditional), which the kernel does not use, so that profiles/det_screen_rate.py can print both.  No GPU, no engine.

The kernel's ring holds the integral image scaled by 2^-10 and w_i carries the 2^10 back; so does the model."""
import numpy as np

SCALE = 2.0 ** -10
SKIP_REL = 2.0 ** -20                            # SD_SKIP_REL
SKIP_ABS = 2.0 ** -18                            # SD_SKIP_ABS
SIZES = (15, 30)


def w_i(size):
    """sd_wi<SIZE>(): 1 / size / size * 2^10"""
    return np.float64(1.0) / np.float64(size) / np.float64(size) * np.float64(1024.0)


def box(Ss, r, c, rl, cl):
    """max(0, ((a + d) - b) - c) over the clipped corners (skimage _integ; the kernel's clamp also caps at 1, which a scaled box sum -
    at most 900 pixels of at most 1.0, times 2^-10 - never reaches)"""
    H, W = Ss.shape
    r, c = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
    r2, c2 = np.clip(r + rl, 0, H - 1), np.clip(c + cl, 0, W - 1)
    t = Ss[np.ix_(r, c)] + Ss[np.ix_(r2, c2)]
    t = t - Ss[np.ix_(r, c2)]
    return np.maximum(t - Ss[np.ix_(r2, c)], 0.0)


def boxes(S, size):
    """(xx_mid, xx_side, yy_mid, yy_side) of every position of the integral image S (unscaled, float64)"""
    Ss = S * SCALE
    H, W = S.shape
    r, c = np.arange(H), np.arange(W)
    s2, s3 = (size - 1) // 2, size // 3
    return (box(Ss, r - s3 + 1, c - s2, 2 * s3 - 1, size), box(Ss, r - s3 + 1, c - s3 // 2, 2 * s3 - 1, s3),
            box(Ss, r - s2, c - s3 + 1, size, 2 * s3 - 1), box(Ss, r - s3 // 2, c - s3 + 1, s3, 2 * s3 - 1))


def deriv(mid, side, size):
    """-(mid - 3 side) w_i, rounded as the kernel rounds it"""
    e = mid - np.float64(3.0) * side
    return (-e) * w_i(size)


def bound(e, mid, size):
    """what |e * d| can reach at most where the product is positive, d = deriv(mid, side) with 0 <= side <= mid unknown"""
    w1 = w_i(size) * np.float64(1.0 + SKIP_REL)
    w2 = np.float64(2.0) * w1
    return (np.abs(e) * mid) * np.where(e > 0.0, w2, w1)


def ruled_out(e, mid, size, thr):
    """the kernel's per-position rule: the unread side box cannot lift e * d above thr"""
    return ~(bound(e, mid, size) > np.float64(thr) - np.float64(SKIP_ABS))


SD_T, SD_OUT, SD_PC, SD_HR = 16, 62, 64, 16     # retrack_geom.h: rows per step, outputs / positions per strip, lowest box row +16


def waves(S, size, thr, exact="dyy"):
    """the screen as the waves of rt_det_strip_kernel see it -> (need, passing, fast): bool (strips, steps, 8, 128) per position of
    wave w8 of a strip's step - position 64 k + lane is row 16 t + 8 k + w8 of column 62 s - 1 + lane, columns outside the image
    clipped as the kernel clips them - need: the position is not ruled out; passing: its product is above thr; and fast: bool
    (steps,), the steps that run sd_tile_fast (the others read every box).  A wave reads the conditional box of the size iff
    need.any(axis=-1)."""
    H, W = S.shape
    ns, nt = -(-W // SD_OUT), H // SD_T + 1
    Ss = S * SCALE
    r, c = np.arange(nt * SD_T), np.arange(-1, SD_OUT * ns + SD_PC - 1)
    s2, s3 = (size - 1) // 2, size // 3
    xm, xs = box(Ss, r - s3 + 1, c - s2, 2 * s3 - 1, size), box(Ss, r - s3 + 1, c - s3 // 2, 2 * s3 - 1, s3)
    ym, ys = box(Ss, r - s2, c - s3 + 1, size, 2 * s3 - 1), box(Ss, r - s3 // 2, c - s3 + 1, s3, 2 * s3 - 1)
    dxx, dyy = deriv(xm, xs, size), deriv(ym, ys, size)
    out = ruled_out(dyy, xm, size, thr) if exact == "dyy" else ruled_out(dxx, ym, size, thr)
    def by_wave(a):
        strips = np.stack([a[:, SD_OUT * s:SD_OUT * s + SD_PC] for s in range(ns)])
        return strips.reshape(ns, nt, 2, 8, SD_PC).transpose(0, 1, 3, 2, 4).reshape(ns, nt, 8, 2 * SD_PC)

    t = np.arange(nt)
    return by_wave(~out), by_wave(dxx * dyy > thr), (t >= 1) & (SD_T * t + SD_T - 1 + SD_HR <= H - 1)


def screen(S, size, thr, exact="dyy"):
    """-> (product dxx * dyy as the kernel rounds it, ruled_out) for every position.  exact = "dyy": the kernel's order (dyy exact, the
    xx-side box conditional); "dxx": the other order"""
    xm, xs, ym, ys = boxes(S, size)
    dxx, dyy = deriv(xm, xs, size), deriv(ym, ys, size)
    out = ruled_out(dyy, xm, size, thr) if exact == "dyy" else ruled_out(dxx, ym, size, thr)
    return dxx * dyy, out
