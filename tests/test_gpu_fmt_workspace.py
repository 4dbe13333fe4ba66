"""GPU (-m gpu): the Fourier-Mellin passes, the phase correlation and a detector share a context's grow-only scratch memory
(csrc/fmt.hip, csrc/phasecorr.hip; roam_scratch frees and reallocates a slot that must grow).  The contract: what a call returns does
not depend on what the context ran before it.  Eight calls on ONE context, in an order that makes the workspace grow, shrink in need
and grow again, with other planes, another chunk size and another unit's use of the same slots between them; every result equals,
bit for bit, that of the same call made first on a context of its own."""
import numpy as np
import pytest

import fmt_register_cases as cases

pytestmark = pytest.mark.gpu


def register(case, **kw):
    _, clip_px, ds, cds, _, _ = cases.CASES[case]
    A, B = cases.batch(case)
    return lambda c: c.fmt_register_batch(A, B, clip_px=clip_px, downsample=ds, cart_downsample=cds, **kw)


def rotation_with_logpolar(case):
    _, clip_px, ds, _, _, _ = cases.CASES[case]
    A, B = cases.batch(case)
    return lambda c: c.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds, want_logpolar=True)


def phase_correlation():
    """47 x 59 -> planes of 48 x 60: none of the registrations' (216 x 64 and 90 x 90, 225 x 72 and 144 x 144, 320 x 108 and 216 x 216)"""
    rng = np.random.default_rng(21)
    a = rng.random((3, 47, 59), dtype=np.float32)
    b = np.roll(a, (2, -3), axis=(1, 2))
    return lambda c: c.phase_correlate(a, b)


def detector():
    img = np.random.default_rng(22).random((64, 64), dtype=np.float32)
    return lambda c: c.doh_maxima(img, [1.0, 2.0, 3.0], 0.001)


def flat(result):
    return [np.asarray(r) for r in (result if isinstance(result, tuple) else (result,))]


def test_results_do_not_depend_on_what_the_context_ran_before(monkeypatch):
    from radarslampy_amd import _ffi
    steps = [           # (what, ROAM_FMT_BATCH_CHUNK or None, the call)
        ("registration tex3", None, register("tex3")),                       # the smallest: Rc 42, planes 90 x 90
        ("registration strided7", None, register("strided7")),
        ("registration live20 with images", None, register("live20", want_images=True)),
        ("phase correlation 47 x 59", None, phase_correlation()),
        ("doh_maxima 64 x 64", None, detector()),
        ("registration tex3, chunk 1", "1", register("tex3")),
        ("registration live20", None, register("live20")),                   # the need shrank, now it grows
        ("rotation live20 with log-polar images", None, rotation_with_logpolar("live20")),
    ]

    def run(c, chunk, call):
        if chunk is None:
            monkeypatch.delenv("ROAM_FMT_BATCH_CHUNK", raising=False)
        else:
            monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", chunk)
        return flat(call(c))

    alone = []
    for what, chunk, call in steps:
        c = _ffi.Context(0)
        alone.append(run(c, chunk, call))
        c.close()
    shared = _ffi.Context(0)
    for (what, chunk, call), want in zip(steps, alone):
        got = run(shared, chunk, call)
        assert len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want)), what
    shared.close()
