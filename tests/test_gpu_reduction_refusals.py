"""The argument checks that the reductions over resident results share (one source resolver, one slot-range check, one window /
bin check), as a table: entry point, bad argument, expected exception.  The engine is 8 x 8, the caller-held arrays are
(2, 3, 64); a refused call launches nothing, an accepted one reduces 384 values.

MSL_ERR_STATE arrives as RuntimeError, MSL_ERR_INVALID as ValueError (pyslice_amd/_native.py: _raise)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, K, B, T = 8, 64, 2, 3
INT_MAX = 2 ** 31 - 1

# how each entry point is called: (engine, src, first slot, count, B)
CALLS = {
    "tacaw_spectrum": lambda e, src, t0, n, b: e.tacaw_spectrum(np.ones(K), src=src),
    "tacaw_spectrum_weighted": lambda e, src, t0, n, b: e.tacaw_spectrum_weighted(np.ones(K), src=src),
    "tacaw_diffraction": lambda e, src, t0, n, b: e.tacaw_diffraction(src=src),
    "tacaw_dispersion": lambda e, src, t0, n, b: e.tacaw_dispersion([0, 5], src=src),
    "adf": lambda e, src, t0, n, b: e.adf(np.ones(K), src=src),
    "detect": lambda e, src, t0, n, b: e.detect(t0, n, B=b, src=src),
    "spectrum_detect": lambda e, src, t0, n, b: e.spectrum_detect(t0, n, B=b, src=src),
    "diffract": lambda e, src, t0, n, b: e.diffract(t0, n, B=b, src=src),
    "coherent_add": lambda e, src, t0, n, b: e.coherent_add(t0, n, B=b, src=src),
    "image_add": lambda e, src, t0, n, b: e.image_add(t0, n, B=b, src=src),
}
INTENSITY = ("tacaw_spectrum", "tacaw_spectrum_weighted", "tacaw_diffraction", "tacaw_dispersion", "spectrum_detect")
SLOTS = ("detect", "spectrum_detect", "diffract", "coherent_add", "image_add")     # the five with a slot range (and a B)
DETECTORS = ("detect", "spectrum_detect")


def source(ctx, name, k=K, ld=None):
    """the src tuple of entry point `name` over the caller-held array of its kind: rows of k pixels, pitch ld (None: not given)"""
    ptr = ctx["I"].data_ptr() if name in INTENSITY else ctx["W"].data_ptr()
    tail = () if ld is None else (ld,)
    if name == "diffract":
        return (ptr, B, T, k // NX, NX) + tail
    if name == "image_add":                                   # rows of nx * ny pixels: no K of its own
        return (ptr, B, T) + tail
    return (ptr, B, T, k) + tail


def raw_slots(e, name, ctx, t0, count):
    """msl_detect / msl_spectrum_detect past their Python wrappers, which size the output by `count` before the library sees
    it; a refused call never writes the output"""
    out = np.empty(1)
    fn = getattr(e._lib, "msl_" + name)
    e._chk(fn(e._h, C.c_void_p(source(ctx, name)[0]), B, T, K, K, t0, count, out.ctypes.data_as(C.c_void_p)))


def table():
    rows = []
    for name in CALLS:
        # NULL source before any result exists: no wavefunction buffer (n_frames = 0), no intensity (no tacaw() yet)
        rows.append((f"{name}-no-resident-result", "empty", lambda e, ctx, c=CALLS[name]: c(e, None, 0, None, None), RuntimeError))
        rows.append((f"{name}-ld-below-K", "full", lambda e, ctx, n=name: CALLS[n](e, source(ctx, n, ld=K - 1), 0, None, None), ValueError))
        rows.append((f"{name}-ld-zero", "full", lambda e, ctx, n=name: CALLS[n](e, source(ctx, n, ld=0), 0, None, None), None))
    for name in SLOTS:
        rows.append((f"{name}-resident-B-above-n_probes", "full", lambda e, ctx, c=CALLS[name]: c(e, None, 0, None, B + 1), ValueError))
        for what, t0, count in [("t0-negative", -1, 1), ("count-zero", 0, 0), ("one-past-the-end", 1, T), ("sum-overflows-int32", 1, INT_MAX)]:
            if name in DETECTORS and count == INT_MAX:
                fn = lambda e, ctx, n=name, t0=t0, count=count: raw_slots(e, n, ctx, t0, count)
            else:
                fn = lambda e, ctx, n=name, t0=t0, count=count: CALLS[n](e, source(ctx, n), t0, count, None)
            rows.append((f"{name}-{what}", "full", fn, ValueError))
    for name in DETECTORS:
        rows.append((f"{name}-K-not-the-detectors", "full", lambda e, ctx, n=name: CALLS[n](e, source(ctx, n, k=K - NX, ld=K), 0, None, None), ValueError))
    rows.append(("diffract-bin-does-not-divide", "full", lambda e, ctx: e.diffract(bin=(3, 1), src=source(ctx, "diffract")), ValueError))
    rows.append(("coherent_finish-bin-does-not-divide", "full", lambda e, ctx: e.coherent_finish(1, bin=(1, 3), shape=(NX, NX)), ValueError))
    return rows


def adf_with_B(e, b):
    """msl_adf on the resident result with a caller's B, which Engine.adf never passes"""
    out = np.empty(B)
    m = np.ones(K, dtype=np.uint8)
    e._chk(e._lib.msl_adf(e._h, None, b, 0, 0, 0, m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))


ROWS = table() + [("adf-resident-B-above-n_probes-is-ignored", "full", lambda e, ctx: adf_with_B(e, B + 1), None)]


@pytest.fixture(scope="module")
def ctx():
    import torch
    from pyslice_amd import _native
    _native.load()
    rng = np.random.default_rng(5)
    W = torch.from_numpy((rng.standard_normal((B, T, K)) + 1j * rng.standard_normal((B, T, K))).astype(np.complex64)).cuda()
    I = torch.from_numpy(rng.random((B, T, K), dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    # "empty": no resident result of either kind; "full": a (zero) wavefunction buffer of 3 frames and its intensity
    engines = {"empty": _native.Engine(NX, NX, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=B, n_frames=0, device=0),
               "full": _native.Engine(NX, NX, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=B, n_frames=T, device=0)}
    k = np.fft.fftfreq(NX).astype(np.float32)
    for e in engines.values():
        e.set_detectors(np.ones(K, dtype=np.uint16), ["intensity"], k, k)
    engines["full"].tacaw()
    engines["full"].coherent_reset(B)
    engines["full"].image_reset(B)
    yield {"W": W, "I": I, **engines}
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("engine,call,expected", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusal_table(ctx, engine, call, expected):
    """The expected classes are those of the code before the checks were single-sourced.  One row differs in kind: with
    t0 = 1, count = 2**31 - 1 that code refused the call through a 64-bit comparison, but three of its five copies then
    formatted t0 + count as an int, a signed overflow (in practice a ValueError with a negative number in its message)."""
    if expected is None:
        call(ctx[engine], ctx)
    else:
        with pytest.raises(expected) as info:
            call(ctx[engine], ctx)
        assert type(info.value) is expected                    # MemoryError and NotImplementedError are other codes
