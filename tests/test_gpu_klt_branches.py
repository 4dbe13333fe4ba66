"""GPU (-m gpu): klt_kernel and the pyramid kernels on the image pairs of tests/klt_branch_cases.py, which take the tracker through its
data-dependent branches (asserted on the CPU by tests/test_klt_branches_cpu.py): unseeded against the oracle, seeded against the
NumPy model, through the u8 and the float32 entry, bit for bit in next, status and err; run twice and split across two calls."""
import numpy as np
import pytest

import klt_branch_cases as B
import klt_flow_model as M
import oracle

pytestmark = pytest.mark.gpu

_truth = {}


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def entries(case):
    """-> [(entry name, prev, next as given to the device, prev, next u8 as the tracker sees them)]: the u8 images, and image / 255 as
    float32, of which the tracker sees oracle.quantize_u8"""
    if ("entries", case["name"]) not in _truth:
        af, bf = (np.ascontiguousarray(x.astype(np.float32) / np.float32(255.)) for x in (case["prev"], case["next"]))
        _truth["entries", case["name"]] = [("u8", case["prev"], case["next"], case["prev"], case["next"]),
                                           ("f32", af, bf, oracle.quantize_u8(af), oracle.quantize_u8(bf))]
    return _truth["entries", case["name"]]


def truth(case, entry):
    """the oracle on its own pyramids (unseeded) or the model (seeded), once per (case, entry)"""
    key = (case["name"], entry[0])
    if key not in _truth:
        a8, b8 = entry[3], entry[4]
        if case["init"] is None:
            _truth[key] = oracle.klt_on_pyramids(oracle.build_pyramid(a8, 3), oracle.build_pyramid(b8, 3), case["pts"])
        else:
            _truth[key] = M.track_on_pyramids(M.build_pyramid(a8), M.build_pyramid(b8), case["pts"], case["init"])
    return _truth[key]


def assert_equal(case, entry, got, want):
    """next, status, err bit for bit; on a difference: the first differing point and the trace classes of its four levels"""
    bad = np.zeros(len(case["pts"]), bool)
    for g, w in zip(got, want):
        bad |= (g.reshape(len(bad), -1).view(np.uint8) != w.reshape(len(bad), -1).view(np.uint8)).any(axis=1)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        seen = dict(case, name=case["name"] + "/" + entry[0], prev=entry[3], next=entry[4])
        pytest.fail("%s %s: %d of %d points differ; first k = %d at %s: device %s, truth %s; its levels (level, exit, classes): %s" % (
            case["name"], entry[0], int(bad.sum()), len(bad), k, case["pts"][k].tolist(), [x[k].tolist() for x in got],
            [x[k].tolist() for x in want], B.point_classes(seen)[k]))


@pytest.mark.parametrize("case", B.unseeded(), ids=lambda c: c["name"])
def test_unseeded_equals_oracle(ctx, case):
    for entry in entries(case):
        want = truth(case, entry)
        got = ctx.klt_track(entry[1], entry[2], case["pts"])
        assert_equal(case, entry, got, want)
        # a seed equal to the points through the _flow entry is the unseeded call
        assert_equal(case, entry, ctx.klt_track(entry[1], entry[2], case["pts"], case["pts"].copy()), want)


@pytest.mark.parametrize("case", B.seeded(), ids=lambda c: c["name"])
def test_seeded_equals_model(ctx, case):
    for entry in entries(case):
        assert_equal(case, entry, ctx.klt_track(entry[1], entry[2], case["pts"], case["init"]), truth(case, entry))


@pytest.mark.parametrize("case", B.cases(), ids=lambda c: c["name"])
def test_pyramid_equals_oracle(ctx, case):
    """level by level; the 0 / 255 images are the no-carry limit of the packed 16-bit column sums"""
    for img in (case["prev"], case["next"]):
        lv = img
        for want in oracle.build_pyramid(img, 3)[1:]:
            lv = ctx.pyr_down_u8(lv)
            assert lv.shape == want.shape and np.array_equal(lv, want), (case["name"], want.shape, int((lv != want).sum()))
        # the tracker's own route to levels 1 and 2 at this width: the builder's two-level branch
        want = oracle.build_pyramid(img, 2)
        offs = [0]
        for a in want[:2]:
            offs.append(offs[-1] + ((a.size + 255) & ~255))
        buf = np.zeros(offs[-1] + ((want[2].size + 255) & ~255), np.uint8)
        buf[:img.size] = img.ravel()
        ctx.pyr_down2_u8(buf, img.shape[1], img.shape[0], 1, buf.size, offs)          # whichever of its kernels the builder picks
        for l in (1, 2):
            got = buf[offs[l]: offs[l] + want[l].size].reshape(want[l].shape)
            assert np.array_equal(got, want[l]), (case["name"], "two-level", l, int((got != want[l]).sum()))
        assert np.array_equal(buf[:img.size], img.ravel())


@pytest.mark.parametrize("case", B.cases(), ids=lambda c: c["name"])
def test_same_bits_twice_and_split(ctx, case):
    """the same call twice, and the points split across two calls (the first alone, then the rest), give the bits of the one call"""
    pts, init = case["pts"], case["init"]
    for entry in entries(case):
        one = ctx.klt_track(entry[1], entry[2], pts, init)
        assert_equal(case, entry, ctx.klt_track(entry[1], entry[2], pts, init), one)
        parts = [ctx.klt_track(entry[1], entry[2], pts[s], None if init is None else init[s]) for s in (slice(0, 1), slice(1, None))]
        assert_equal(case, entry, [np.concatenate(x) for x in zip(*parts)], one)
