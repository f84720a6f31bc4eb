"""Spectrum imaging on the host: the Spectroscopy request, the refusals of the calculator, the memory rule on literal free-byte
values, the engine calls of run_spectrum_image() on an engine that only records them, SpectrumImageData on a hand-made array, and
the ABI entry."""
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = [(0.3 * i, 0.2 * i) for i in range(5)]
GRID = "32, 32, 3, 0.0984375, 0.0984375, 0.416666666667, 0.0370143628314, 0.000924395920681"      # nx, ny, nz, dx, dy, dz, wavelength, sigma


class SpectrumEngine(RecordingEngine):
    """RecordingEngine that answers spectrum_detect with a (B, T, D) array: 1000 * call number + the row's place in the call"""

    def spectrum_detect(self, *a, **k):
        self.calls.append(("spectrum_detect", a, k))
        n = sum(1 for c in self.calls if c[0] == "spectrum_detect")
        return 1000.0 * n + np.arange(k["B"], dtype=np.float64)[:, None, None] + np.zeros((k["B"], self.n_frames, self._D))


def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def _dets():
    from pyslice_amd import Detector
    return [Detector("bf", outer=20.0), Detector("adf", inner=40.0)]


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


def _no_engine(*a, **k):
    raise AssertionError("device work before the check")


# ------------------------------------------------------------------ 1. the ABI
def test_spectrum_detect_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"\bmsl_spectrum_detect\s*\(", hdr)
    assert "msl_spectrum_detect" in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr) and _native.ABI_VERSION == 3
    assert callable(_native.Engine.spectrum_detect)


# ------------------------------------------------------------------ 2. the request
def test_spectroscopy_validation():
    from pyslice_amd import Detector, Spectroscopy
    sp = Spectroscopy(_dets())
    assert [d.name for d in sp.detectors] == ["bf", "adf"] and sp.stem is False
    assert Spectroscopy(detectors=_dets(), stem=True).stem is True
    assert len(Spectroscopy([Detector(f"d{i}") for i in range(16)]).detectors) == 16
    with pytest.raises(ValueError, match="at most 16"):
        Spectroscopy([Detector(f"d{i}") for i in range(17)])
    with pytest.raises(ValueError):
        Spectroscopy([])
    with pytest.raises(ValueError, match="duplicate"):
        Spectroscopy([Detector("a"), Detector("a", inner=10.0)])
    with pytest.raises(ValueError):
        Spectroscopy(["adf"])
    for signal in ("amplitude", "com_x", "com_y"):
        with pytest.raises(ValueError, match="intensity"):
            Spectroscopy([Detector("bf", outer=10.0), Detector("x", signal=signal)])
    with pytest.raises(ValueError, match="stem"):
        Spectroscopy(_dets(), stem=1)


# ------------------------------------------------------------------ 3. refusals, before any device work
def test_constructor_refusals(monkeypatch):
    from pyslice_amd import Aberrations, Diffraction, Imaging, Spectroscopy, _native
    from pyslice_amd.prism import Prism
    monkeypatch.setattr(_native, "Engine", _no_engine)
    sp = Spectroscopy(_dets())
    for kw in (dict(detectors=_dets()), dict(diffraction=Diffraction(bin=(2, 2))), dict(imaging=Imaging()), dict(prism=Prism((1, 1))),
               dict(layers=[1]), dict(cache=True), dict(stream_tile=4), dict(k_bin=(2, 2))):
        with pytest.raises(ValueError, match="spectroscopy"):
            _calc(spectroscopy=sp, **kw)
    with pytest.raises(ValueError, match="spectroscopy"):
        _calc(spectroscopy=_dets())
    with pytest.raises(ValueError, match="probe_batch"):
        _calc(spectroscopy=sp, probe_batch=0)
    with pytest.raises(ValueError, match="detectors"):                 # (the existing refusal and its text stay)
        _calc(probe_batch=8)
    _calc(spectroscopy=sp, k_window=(16, 16), aberrations=Aberrations(defocus=50.0), frame_batch=2, probe_batch=3)


def test_run_modes_name_each_other(monkeypatch):
    from pyslice_amd import Detector, Spectroscopy, _native
    monkeypatch.setattr(_native, "Engine", _no_engine)
    calc = _calc(spectroscopy=Spectroscopy(_dets()))
    for method in ("run", "run_detectors", "run_diffraction", "run_images"):
        with pytest.raises(RuntimeError, match="run_spectrum_image"):
            getattr(calc, method)()
    with pytest.raises(RuntimeError, match="setup"):
        calc.run_spectrum_image()
    for other in (_calc(), _calc(detectors=[Detector("bf", outer=10.0)])):
        with pytest.raises(RuntimeError, match="spectroscopy"):
            other.run_spectrum_image()


def test_setup_refusals_before_device_work(monkeypatch):
    from pyslice_amd import Detector, Spectroscopy, _native, distributed
    monkeypatch.setattr(_native, "Engine", _no_engine)
    calc = _calc(spectroscopy=Spectroscopy(_dets()))
    with pytest.raises(ValueError, match="2 frames"):
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3)
    assert calc._engine is None
    calc = _calc(spectroscopy=Spectroscopy([Detector("bf", outer=10.0), Detector("far", inner=5000.0)]))
    with pytest.raises(ValueError, match="far"):
        calc.setup(_trajectory(3), aperture=30.0, voltage_eV=100e3)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    calc = _calc(spectroscopy=Spectroscopy(_dets()))
    with pytest.raises(NotImplementedError, match="ranks"):
        calc.setup(_trajectory(3), aperture=30.0, voltage_eV=100e3)
    assert calc._engine is None


# ------------------------------------------------------------------ 4. the memory rule
def _sized(monkeypatch, free_b, n_frames=8, **kw):
    """the (n_probes, n_frames, frame_batch) of the engine setup() creates for 5 probes at `free_b` free bytes"""
    from pyslice_amd import Spectroscopy, _native, calculators
    monkeypatch.setattr(_native, "Engine", SpectrumEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: free_b)
    calc = _calc(spectroscopy=Spectroscopy(_dets()), **kw)
    calc.setup(_trajectory(n_frames), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    eng = calc._engine
    return calc, (eng.n_probes, eng.n_frames, eng.frame_batch)


def test_memory_rule_on_literal_free_bytes(monkeypatch):
    """32 x 32 grid (pitch 1024), 3 slices, 2 atoms, T = 8 frames, frame batch 8.  Per probe: the ring and the intensity with T
    slots, 8 * 1024 * (8 + 4) = 98304 bytes, and the work buffers of the frame batch, 8 * 32 * 1024 = 262144; fixed: the stacks
    8 * 16 * 3 * 1024 = 393216, the phase tables 8 * 2 * 34 * 8 = 4352 and 1e9."""
    fixed = 393216 + 4352 + 1e9
    per_probe = 98304 + 262144
    calc, sized = _sized(monkeypatch, 300e9)
    assert sized == (5, 8, 8)                                          # the ring has T slots, the potentials a frame batch
    assert calc.probe_batch == 5
    fit = calc._fit_spectrum_batch
    assert fit(300e9, 5, 8) == 5
    assert fit((fixed + 5 * per_probe) / 0.9 + 1.0, 5, 8) == 5
    assert fit((fixed + 5 * per_probe) / 0.9 - 1.0, 5, 8) == 2        # halved
    assert fit((fixed + 2 * per_probe) / 0.9 - 1.0, 5, 8) == 1
    assert fit((fixed + 1 * per_probe) / 0.9 + 1.0, 5, 8) == 1
    with pytest.raises(MemoryError, match="k_window"):
        fit((fixed + 1 * per_probe) / 0.9 - 1.0, 5, 8)
    # the ring is counted with T slots, not with the frame batch: at a frame batch of 2 the per-probe ring term stays 98304
    fixed2 = 2 * 16 * 3 * 1024 + 2 * 2 * 34 * 8 + 1e9
    per2 = 98304 + 2 * 32 * 1024
    assert fit((fixed2 + 5 * per2) / 0.9 + 1.0, 5, 2) == 5
    assert fit((fixed2 + 5 * per2) / 0.9 - 1.0, 5, 2) == 2
    # setup() applies the rule to the default probe batch ...
    assert _sized(monkeypatch, (fixed + 5 * per_probe) / 0.9 - 1.0)[1] == (2, 8, 8)
    with pytest.raises(MemoryError, match="k_window"):
        _sized(monkeypatch, 1.0e9)
    # ... a k_window shrinks the ring (pitch 128: 8 * 128 * 12 = 12288 per probe) ...
    calc, sized = _sized(monkeypatch, 300e9, k_window=(16, 8))
    assert sized == (5, 8, 8)
    assert calc._fit_spectrum_batch((fixed + 5 * (12288 + 262144)) / 0.9 + 1.0, 5, 8) == 5
    # ... and an explicit probe_batch is honoured as it is
    assert _sized(monkeypatch, 1.0, probe_batch=4)[1] == (4, 8, 8)
    assert _sized(monkeypatch, None, probe_batch=2, frame_batch=3)[1] == (2, 8, 3)


# ------------------------------------------------------------------ 5. the loop
def _trace(monkeypatch, frame_batch, stem=False):
    from pyslice_amd import Spectroscopy, _native, calculators
    monkeypatch.setattr(_native, "Engine", SpectrumEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    calc = _calc(spectroscopy=Spectroscopy(_dets(), stem=stem), probe_batch=2, frame_batch=frame_batch)
    calc.setup(_trajectory(5), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    res = calc.run_spectrum_image()
    eng = calc._engine
    lines = format_calls([eng.created] + eng.calls, PP)
    return res, [lines[0].replace(GRID, "GRID")] + lines[1:]


SETUP = ["set_kirkland(f8(103,3,4))", "set_slices(f8(3,), f8(3,))", "set_aberrations(None)",
         "set_detectors(u2(1024,), (intensity,intensity), f4(32,), f4(32,))"]
FRAMES_FB2 = ["build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "build_potentials(f8(2,2,3), i4(2,), 2)",
              "propagate_frames(2, 2)", "build_potentials(f8(1,2,3), i4(2,), 2)", "propagate_frames(4, 1)"]


def test_engine_calls_of_the_loop(monkeypatch):
    """P = 5 at probe_batch 2, T = 5 at frame_batch 2: three probe batches, the last padded; the frame batches go to slots 0, 2, 4;
    one tacaw and one spectrum_detect(B=real) per probe batch; the potentials are built once per probe batch"""
    res, lines = _trace(monkeypatch, 2)
    want = ["Engine(GRID, n_probes=2, n_frames=5, frame_batch=2, window=None, k_bin=None, device=0)"] + SETUP
    for xy, real in (("xy[0,1]", 2), ("xy[2,3]", 2), ("xy[4,4]", 1)):
        want += [f"set_probes(30, {xy})"] + FRAMES_FB2 + ["tacaw()", f"spectrum_detect(B={real})"]
    assert lines == want
    assert sum(line.startswith("build_potentials") for line in lines) == 3 * 3
    # the rows of every spectrum_detect land at p0 .. p0+real-1
    assert res.spectra.shape == (5, 5, 2) and res.stem is None
    assert res.spectra[:, 0, 0].tolist() == [1000.0, 1001.0, 2000.0, 2001.0, 3000.0]
    assert np.array_equal(res.frequencies, np.fft.fftshift(np.fft.fftfreq(5, _trajectory(5).timestep)))
    assert res.n_frames == 5 and [d.name for d in res.detectors] == ["bf", "adf"]


def test_one_frame_batch_builds_the_potentials_once(monkeypatch):
    res, lines = _trace(monkeypatch, 8, stem=True)
    want = ["Engine(GRID, n_probes=2, n_frames=5, frame_batch=5, window=None, k_bin=None, device=0)"] + SETUP
    want += ["build_potentials(f8(5,2,3), i4(2,), 2)"]
    for xy, real in (("xy[0,1]", 2), ("xy[2,3]", 2), ("xy[4,4]", 1)):
        want += [f"set_probes(30, {xy})", "propagate_frames(0, 5)", "tacaw()", f"spectrum_detect(B={real})", f"detect(0, 5, B={real})"]
    assert lines == want
    assert res.stem is not None and res.stem.signals.shape == (5, 5, 2)


def test_frames_inside_loop_default_keeps_slot_zero():
    """the keyword's default leaves the split / imaging loops as they were (tests/test_calculator_host.py pins their calls)"""
    import inspect
    from pyslice_amd.calculators import MultisliceCalculator
    assert inspect.signature(MultisliceCalculator._frames_inside_loop).parameters["own_slots"].default is False


# ------------------------------------------------------------------ 6. SpectrumImageData
def test_spectrum_image_data_accessors():
    from pyslice_amd import Detector, SpectrumImageData
    rng = np.random.default_rng(3)
    xs0, ys0 = np.linspace(1.0, 5.0, 3), np.linspace(0.5, 4.0, 4)
    pp = np.array([(x, y) for x in xs0 for y in ys0])[rng.permutation(12)]
    T, dt = 8, 0.005
    freqs = np.fft.fftshift(np.fft.fftfreq(T, dt))                 # -100, -75, ..., 75
    S = rng.random((12, T, 2))
    d = SpectrumImageData(spectra=S, frequencies=freqs, detectors=[Detector("a"), Detector("b", inner=10.0)], probe_positions=pp, n_frames=T)
    assert np.array_equal(d.xs, xs0) and np.array_equal(d.ys, ys0) and d.stem is None and d.n_frames == T
    # the probe mean and one probe
    assert np.array_equal(d.spectrum("b"), S[:, :, 1].mean(axis=0))
    assert np.array_equal(d.spectrum("a", 7), S[7, :, 0])
    with pytest.raises(ValueError):
        d.spectrum("a", 12)
    with pytest.raises(KeyError):
        d.spectrum("c")
    # the nearest bin: 30 -> 25 (index 5), -90 -> -100 (index 0); placed on the scan grid by the nearest probe
    def grid(per):
        return np.array([[per[np.argmin(((pp - (x, y)) ** 2).sum(1))] for y in ys0] for x in xs0])
    assert np.array_equal(d.image("b", frequency=30.0), grid(S[:, 5, 1]))
    assert np.array_equal(d.image("a", frequency=-90.0), grid(S[:, 0, 0]))
    assert d.image("a", frequency=0.0).shape == (3, 4)
    # the band sum includes both edges: [-50, 25] = bins 2 .. 5
    assert np.array_equal(d.image("b", band=(-50.0, 25.0)), grid(S[:, 2:6, 1].sum(axis=1)))
    assert np.array_equal(d.per_probe("a", band=(25.0, 25.0)), S[:, 5, 0])
    with pytest.raises(ValueError):
        d.image("a", band=(26.0, 49.0))
    with pytest.raises(ValueError):
        d.image("a")
    with pytest.raises(ValueError):
        d.image("a", frequency=1.0, band=(0.0, 1.0))
    with pytest.raises(ValueError, match="shape"):
        SpectrumImageData(spectra=S[:, :4], frequencies=freqs, detectors=d.detectors, probe_positions=pp, n_frames=T)
