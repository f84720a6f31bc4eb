"""Windowed, segment-averaged (Welch) TACAW spectra, the part that needs no device: the float64 definition (pyslice_amd/welch.py)
against the oracle's periodogram and scipy.signal.welch, the segment and window rules, the header and the binding, the refusals of
TACAWData and Spectroscopy, and the engine calls of run_spectrum_image() with a segment."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import rel_l2
from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = 1e-12
LENGTHS = [16, 18, 20, 21, 24, 25, 27, 28, 30, 32, 35, 36, 40, 42, 45, 48, 49, 50, 54, 56, 60, 63, 64, 70, 72, 75, 80, 81, 84, 90, 96, 98,
           100, 105, 108, 112, 120, 125, 126, 128]
PP = [(0.3 * i, 0.2 * i) for i in range(5)]


# ------------------------------------------------------------------ 1. the definition
def test_one_boxcar_segment_is_the_reference_transform(golden):
    from oracle import multislice_oracle as orc
    from pyslice_amd import welch
    g = golden("g8_tacaw_32")
    wf = g["wavefunction_data"]
    if wf.ndim == 5:
        wf = wf[..., -1]
    T = wf.shape[1]
    _, want = orc.tacaw(g["wavefunction_data"], g["time"])
    got = welch.welch_intensity(wf, T, T, "boxcar")
    assert got.shape == np.asarray(want).shape
    assert rel_l2(got, want) <= TOL64


@pytest.mark.parametrize("name", ["boxcar", "hann", "hamming", "blackman"])
@pytest.mark.parametrize("L,hop", [(48, 24), (32, 32), (25, 12), (64, 20)])
def test_equals_scipy_welch_outside_bin_zero(name, L, hop):
    signal = pytest.importorskip("scipy.signal")
    from pyslice_amd import welch
    rng = np.random.default_rng(L * 100 + hop)
    T = 96
    x = 3.0 + rng.standard_normal((2, T, 5)) + 1j * rng.standard_normal((2, T, 5))
    got = welch.welch_intensity(x, L, hop, name)
    _, pxx = signal.welch(x, fs=1.0, window=name, nperseg=L, noverlap=L - hop, detrend="constant", return_onesided=False,
                          scaling="density", axis=1)
    want = np.fft.fftshift(pxx * L, axes=1)
    keep = np.arange(L) != L // 2                      # (bin 0 sits at L // 2 of the shifted axis)
    assert np.array_equal(got[:, L // 2], np.zeros((2, 5)))
    assert rel_l2(got[:, keep], want[:, keep]) <= TOL64
    assert np.array_equal(welch.window(name, L), welch.window(name, L)) and np.allclose(welch.window(name, L), signal.get_window(name, L), rtol=0, atol=1e-15)


def test_segment_counts():
    from pyslice_amd import welch
    assert welch.segments(48, 48, 24) == 1
    assert welch.segments(144, 48, 48) == 3
    assert welch.segments(96, 48, 24) == 3
    assert welch.segments(100, 48, 20) == 3             # frames 88 .. 99 are a tail that no full segment covers
    assert welch.segments(100, 48, 1) == 53
    for bad in ((48, 49, 10), (48, 16, 0), (48, 16, 17), (1, 1, 1)):
        with pytest.raises(ValueError):
            welch.segments(*bad)
    assert welch.hop_of(48, 0.5) == 24 and welch.hop_of(25, 0.5) == 13 and welch.hop_of(16, 0.0) == 16 and welch.hop_of(16, 0.99) == 1
    for bad in (-0.1, 1.0, 1.5, "half", None, True):
        with pytest.raises(ValueError, match="overlap"):
            welch.hop_of(16, bad)


def test_windows_are_periodic():
    from pyslice_amd import welch
    for L in (16, 48, 128):
        h = welch.window("hann", L)
        assert h[0] == 0.0 and h[L // 2] == 1.0 and h.shape == (L,)
        assert np.allclose(h[1:], h[1:][::-1], rtol=0, atol=1e-15)        # DFT-even: w[n] = w[L - n]
    assert np.array_equal(welch.window("boxcar", 25), np.ones(25)) and np.array_equal(welch.window(None, 25), np.ones(25))
    arr = np.linspace(0.0, 1.0, 20)
    assert np.array_equal(welch.window(arr, 20), arr)
    for bad in ("kaiser", np.ones(19), -np.ones(20), np.zeros(20), np.full(20, np.nan), object()):
        with pytest.raises(ValueError):
            welch.window(bad, 20)


def test_named_windows_are_never_negative():
    """msl_tacaw_welch refuses a negative window value, and a named window is itself a valid array window: at every supported
    length (blackman's 0.42 - 0.5 + 0.08 at n = 0 rounds below zero unless it is clamped)"""
    from pyslice_amd import welch
    for name in welch.WINDOWS:
        for L in welch.supported_lengths():
            w = welch.window(name, L)
            assert w.min() >= 0.0 and np.sum(w * w) > 0, (name, L, w.min())
            assert np.array_equal(welch.window(w, L), w)
    assert welch.window("blackman", 48)[0] == 0.0


def test_an_offset_does_not_leak_through_the_window():
    """what the segment mean is for: under a Hann window a constant that is NOT removed leaks into bins +-1"""
    from pyslice_amd import welch
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 64, 3)) + 1j * rng.standard_normal((1, 64, 3))
    a = welch.welch_intensity(x, 32, 16, "hann")
    b = welch.welch_intensity(x + (4096.0 - 1000.0j), 32, 16, "hann")
    assert rel_l2(b, a) <= 1e-9                        # (float64 cancellation of a 4096 offset: about 4096 * 1e-16 * sqrt(L))


# ------------------------------------------------------------------ 2. the lengths, the header, the binding
def test_supported_lengths():
    from pyslice_amd import welch
    assert welch.supported_lengths() == LENGTHS and len(LENGTHS) == 40
    assert welch.nearest_supported(100) == (100, 100)
    assert welch.nearest_supported(33) == (32, 35)
    assert welch.nearest_supported(200) == (128, None) and welch.nearest_supported(3) == (None, 16)


def test_library_has_a_kernel_for_exactly_these_lengths():
    from pyslice_amd import _native, build_native
    build_native.build()
    assert [L for L in range(1, 201) if _native.welch_has(L)] == LENGTHS
    assert not _native.welch_has(0) and not _native.welch_has(-16)


def test_header_and_binding():
    from pyslice_amd import _native, build_native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int msl_tacaw_welch_has(int32_t L);" in flat
    assert ("int msl_tacaw_welch(msl_handle* h, const void* d_src_c64, void* d_dst_f32, int64_t batch, int32_t T, int64_t npix, "
            "int32_t L, int32_t hop, const double* window_L);") in flat
    assert "int msl_tacaw_welch_layer(msl_handle* h, int32_t layer, int32_t L, int32_t hop, const double* window_L);" in flat
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr) and _native.ABI_VERSION == 3
    for name in ("msl_tacaw_welch_has", "msl_tacaw_welch", "msl_tacaw_welch_layer"):
        assert name in _native.EXPORTS
    build_native.build()
    lib = _native.load()
    assert lib.msl_abi_version() == 3
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.msl_tacaw_welch_has.argtypes == [i32] and lib.msl_tacaw_welch_has.restype == C.c_int
    assert lib.msl_tacaw_welch.argtypes == [vp, vp, vp, i64, i32, i64, i32, i32, vp] and lib.msl_tacaw_welch.restype == C.c_int
    assert lib.msl_tacaw_welch_layer.argtypes == [vp, i32, i32, i32, vp] and lib.msl_tacaw_welch_layer.restype == C.c_int
    assert callable(_native.Engine.tacaw_welch) and callable(_native.Engine.tacaw_welch_layer)
    assert "tacaw_welch.hip" in build_native.SOURCES


# ------------------------------------------------------------------ 3. refusals, before any device work
def _no_engine(*a, **k):
    raise AssertionError("device work before the check")


def _wf(T=32):
    """a WFData assembled on the host: (2, T, 4, 4, 1) waves"""
    from pyslice_amd import WFData
    rng = np.random.default_rng(1)
    data = rng.standard_normal((2, T, 4, 4, 1)) + 1j * rng.standard_normal((2, T, 4, 4, 1))
    ax = np.fft.fftshift(np.fft.fftfreq(4, 0.5))
    return WFData(probe_positions=[(0.0, 0.0), (1.0, 1.0)], time=np.arange(T) * 0.005, kxs=ax, kys=ax, layer=np.array([0]),
                  wavefunction_data=data, probe=None)


def test_tacaw_data_refusals(monkeypatch):
    from pyslice_amd import TACAWData, _native
    monkeypatch.setattr(_native, "Engine", _no_engine)
    with pytest.raises(ValueError, match=r"\b32 and 35\b"):
        TACAWData(_wf(64), segment=33)                              # unsupported: names the two nearest lengths
    with pytest.raises(ValueError, match="128"):
        TACAWData(_wf(64), segment=256)
    with pytest.raises(ValueError, match="exceeds the 32 frames"):
        TACAWData(_wf(32), segment=48)                              # L > T
    for overlap in (-0.25, 1.0, 2.0):
        with pytest.raises(ValueError, match="overlap"):
            TACAWData(_wf(32), segment=16, overlap=overlap)
    for window in ("kaiser", np.ones(15), -np.ones(16), np.zeros(16)):
        with pytest.raises(ValueError, match="window"):
            TACAWData(_wf(32), segment=16, window=window)
    with pytest.raises(ValueError, match="integer"):
        TACAWData(_wf(32), segment=16.0)


def test_tacaw_data_refuses_a_frame_sharded_result(monkeypatch):
    from pyslice_amd import TACAWData
    wf = _wf(32)
    wf._engine, wf._frame_shard = object(), (32, 16)
    with pytest.raises(NotImplementedError, match="is not built"):
        TACAWData(wf, segment=16)


def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def _dets():
    from pyslice_amd import Detector
    return [Detector("bf", outer=20.0), Detector("adf", inner=40.0)]


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


def test_spectroscopy_refusals(monkeypatch):
    from pyslice_amd import Spectroscopy, _native
    monkeypatch.setattr(_native, "Engine", _no_engine)
    sp = Spectroscopy(_dets(), segment=16)
    assert (sp.segment, sp.hop) == (16, 8) and np.array_equal(sp.window, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(16) / 16))
    assert Spectroscopy(_dets(), segment=25, overlap=0.0, window="boxcar").hop == 25
    plain = Spectroscopy(_dets(), overlap=7.0, window="nonsense")       # without a segment both are ignored
    assert plain.segment is None and plain.hop is None and plain.window is None
    with pytest.raises(ValueError, match=r"\b16 and 18\b"):
        Spectroscopy(_dets(), segment=17)
    with pytest.raises(ValueError, match="128"):
        Spectroscopy(_dets(), segment=130)
    for overlap in (-0.1, 1.0):
        with pytest.raises(ValueError, match="overlap"):
            Spectroscopy(_dets(), segment=16, overlap=overlap)
    for window in ("kaiser", np.ones(3), -np.ones(16), np.zeros(16)):
        with pytest.raises(ValueError, match="window"):
            Spectroscopy(_dets(), segment=16, window=window)
    calc = _calc(spectroscopy=Spectroscopy(_dets(), segment=16))
    with pytest.raises(ValueError, match="exceeds the 8 frames"):
        calc.setup(_trajectory(8), aperture=30.0, voltage_eV=100e3)     # L > T, in setup(), before any device work
    assert calc._engine is None


# ------------------------------------------------------------------ 4. the loop
class WelchEngine(RecordingEngine):
    """RecordingEngine whose tacaw_welch sets the frequency count, and whose spectrum_detect answers with (B, F, D)"""

    def tacaw_welch(self, L, hop, window=None, **k):
        self.calls.append(("tacaw_welch", (L, hop, window), k))
        self._F = L

    def spectrum_detect(self, *a, **k):
        self.calls.append(("spectrum_detect", a, k))
        n = sum(1 for c in self.calls if c[0] == "spectrum_detect")
        return 1000.0 * n + np.arange(k["B"], dtype=np.float64)[:, None, None] + np.zeros((k["B"], self._F, self._D))


@pytest.mark.parametrize("stem", [False, True])
def test_run_spectrum_image_calls_tacaw_welch_once_per_probe_batch(monkeypatch, stem):
    from pyslice_amd import Spectroscopy, _native, calculators
    monkeypatch.setattr(_native, "Engine", WelchEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    T, L = 20, 16
    calc = _calc(spectroscopy=Spectroscopy(_dets(), stem=stem, segment=L, overlap=0.5, window="hamming"), probe_batch=2, frame_batch=20)
    tr = _trajectory(T)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    res = calc.run_spectrum_image()
    names = [c[0] for c in calc._engine.calls]
    assert "tacaw" not in names and names.count("tacaw_welch") == 3 and names.count("spectrum_detect") == 3
    lines = format_calls(calc._engine.calls, PP)
    want = []
    for xy, real in (("xy[0,1]", 2), ("xy[2,3]", 2), ("xy[4,4]", 1)):
        want += [f"set_probes(30, {xy})", f"propagate_frames(0, {T})", "tacaw_welch(16, 8, f8(16,))", f"spectrum_detect(B={real})"]
        want += [f"detect(0, {T}, B={real})"] if stem else []
    assert [l for l in lines if not l.startswith(("set_kirkland", "set_slices", "set_aberrations", "set_detectors", "build_potentials"))] == want
    for c in calc._engine.calls:
        if c[0] == "tacaw_welch":
            assert np.array_equal(c[1][2], 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(L) / L))
    assert res.spectra.shape == (5, L, 2)
    assert res.spectra[:, 0, 0].tolist() == [1000.0, 1001.0, 2000.0, 2001.0, 3000.0]
    assert np.array_equal(res.frequencies, np.fft.fftshift(np.fft.fftfreq(L, tr.timestep)))
    assert res.n_frames == T
    assert (res.stem is not None and res.stem.signals.shape == (5, T, 2)) if stem else res.stem is None
