"""PRISM on the cropped window grid, on the host: the fold identity fft2(psi_c) = fft2(psi_p)[::fx, ::fy] in float64, crop_index,
the Prism(crop=) argument, and the calculator's two engines -- call order, validation against the cropped grid, the batch fit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from recording_engine import RecordingEngine, format_calls

from oracle import multislice_oracle as orc
from pyslice_amd import prism
from pyslice_amd.prism import Prism

EV = 100e3
LAM = orc.wavelength(EV)
D = 0.1
# (nx, ny, f): even / even, unequal interpolations, and an odd 45 x 35 cropped grid
GRIDS = [(64, 64, (2, 2)), (96, 80, (2, 4)), (90, 70, (2, 2))]


def positions(nx, ny, n=5):
    """the window of the first position wraps the cell edge on both axes (the probe peaks at pixel (0, 1)), the second lies half a
    pixel off the grid on both, the third wraps along x only; the rest are scattered"""
    rng = np.random.default_rng(nx * 1000 + ny)
    fixed = [(nx * D / 2, ny * D / 2 - D), (1.25, 0.35), (nx * D / 2 + 0.3, 0.7)]
    rest = rng.uniform(0.0, 1.0, (max(0, n - len(fixed)), 2)) * [nx * D, ny * D]
    return np.concatenate([np.array(fixed), rest])[:n]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _aberrations():
    from pyslice_amd.aberrations import Aberrations
    return Aberrations(defocus=-150.0, Cs=2.0e5, astigmatism=40.0, astigmatism_angle=0.3)


@pytest.mark.parametrize("aberrated", [False, True])
@pytest.mark.parametrize("nx,ny,f", GRIDS)
def test_fold_identity_and_parseval(nx, ny, f, aberrated):
    fx, fy = f
    hxhy = prism.beams(nx, ny, D, D, 30.0, LAM, f)
    rng = np.random.default_rng(7)
    S = rng.standard_normal((len(hxhy), nx, ny)) + 1j * rng.standard_normal((len(hxhy), nx, ny))
    xy = positions(nx, ny)
    ab = _aberrations() if aberrated else None
    full = prism.prism_waves(S, hxhy, xy, D, D, f, LAM, ab)
    crop = prism.prism_waves_cropped(S, hxhy, xy, D, D, f, LAM, ab)
    assert crop.shape == (len(xy), nx // fx, ny // fy)
    # the windows of the fixed positions do what their names say
    wrap_x = prism.window_mask(nx, D, xy[0, 0], fx)
    wrap_y = prism.window_mask(ny, D, xy[0, 1], fy)
    assert wrap_x[0] and wrap_x[-1] and not wrap_x.all() and wrap_y[0] and wrap_y[-1] and not wrap_y.all()
    assert abs(xy[1, 0] / D - np.floor(xy[1, 0] / D) - 0.5) < 1e-9 and abs(xy[1, 1] / D - np.floor(xy[1, 1] / D) - 0.5) < 1e-9
    # the fold is a permutation of the window's pixels
    assert np.allclose(np.sort(np.abs(crop).ravel()), np.sort(np.abs(full)[np.abs(full) > 0].ravel()), rtol=0, atol=0)
    F, Fc = np.fft.fft2(full), np.fft.fft2(crop)
    assert _rel(Fc, F[:, ::fx, ::fy]) < 1e-12
    ix, iy = prism.crop_index(nx, fx), prism.crop_index(ny, fy)
    shifted = np.fft.fftshift(F, axes=(1, 2))
    assert _rel(np.fft.fftshift(Fc, axes=(1, 2)), shifted[:, ix[:, None], iy[None, :]]) < 1e-12
    # Parseval: every cropped pixel stands for fx fy full ones
    for p in range(len(xy)):
        assert abs((np.abs(F[p]) ** 2).sum() / (fx * fy * (np.abs(Fc[p]) ** 2).sum()) - 1.0) < 1e-12


@pytest.mark.parametrize("n,f", [(64, 2), (96, 2), (80, 4), (90, 2), (70, 2), (45, 3), (63, 1), (64, 64)])
def test_crop_index(n, f):
    idx = prism.crop_index(n, f)
    w = n // f
    assert idx.shape == (w,) and idx.dtype == np.int64
    assert idx.min() >= 0 and idx.max() < n and np.all(np.diff(idx) == f)
    assert idx[w // 2] == n // 2                                            # DC onto DC
    # the frequencies of the kept pixels are the cropped grid's own axis
    full = np.fft.fftshift(np.fft.fftfreq(n, D))
    assert np.allclose(full[idx], np.fft.fftshift(np.fft.fftfreq(w, D)), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        prism.crop_index(n, 0)
    if n % 7:
        with pytest.raises(ValueError):
            prism.crop_index(n, 7)


def test_prism_crop_argument_and_repr():
    assert Prism(2).crop is False and not Prism(2).cropped
    assert Prism(2, crop=True).crop is True and Prism(2, crop=True).cropped and Prism((1, 2), crop=True).cropped
    assert Prism(1, crop=True).crop is True and not Prism(1, crop=True).cropped      # nothing to crop: runs as crop=False
    assert repr(Prism((2, 4), crop=True)) == "Prism(interpolation=(2, 4), crop=True)"
    assert repr(Prism(2)) == "Prism(interpolation=(2, 2), crop=False)"
    for bad in (1, 0, "yes", None, (True,)):
        with pytest.raises(ValueError, match="crop"):
            Prism(2, crop=bad)
    with pytest.raises(ValueError):
        Prism(0, crop=True)


# ---- the calculator ---------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (4.8, 0.4), (0.0, 0.0), (2.5, 2.5), (3.1, 0.9)]


class LoggedEngine(RecordingEngine):
    """RecordingEngine that also keeps every instance, and every call of all of them in one ordered log"""
    made, log = [], []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.role = "beam" if self.n_frames == 0 else "result"
        LoggedEngine.made.append(self)

    def __getattr__(self, name):
        call = RecordingEngine.__getattr__(self, name)

        def logged(*a, **k):
            LoggedEngine.log.append((self.role, name))
            out = call(*a, **k)
            if name == "set_polar":
                self._bins = int(a[1])
            if name == "polar_detect":
                return np.zeros((k["B"], a[1], self._bins))
            return out
        return logged


@pytest.fixture(scope="module")
def traj():
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(96, 6, 2, ny=80, density=0.05, seed=4, species=(79,))


def _calc(**kw):
    import pyslice_amd as ps
    return ps.MultisliceCalculator(device=0, progress=False, **kw)


def _adf():
    from pyslice_amd.stem_data import Detector
    return [Detector("adf", inner=40.0, outer=120.0)]


def _recorded(monkeypatch, traj, run, **kw):
    from pyslice_amd import _native
    LoggedEngine.made, LoggedEngine.log = [], []
    monkeypatch.setattr(_native, "Engine", LoggedEngine)
    calc = _calc(**kw)
    calc.setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    out = getattr(calc, run)()
    return calc, out, [format_calls([e.created] + e.calls, PP) for e in LoggedEngine.made]


def test_call_order_of_a_cropped_detector_run(traj, monkeypatch):
    """2 frames, 5 probes, probe_batch = 2: the beam engine on the full grid without a result, the result engine on the cropped grid
    without a potential; per frame one potential and one S-matrix, three cropped probe batches, each reduced on the result engine"""
    calc, out, (beam, result) = _recorded(monkeypatch, traj, "run_detectors", detectors=_adf(), probe_batch=2, prism=Prism(2, crop=True))
    assert len(LoggedEngine.made) == 2 and calc._engine is LoggedEngine.made[1] and calc._beam_engine is LoggedEngine.made[0]
    assert beam[0].startswith("Engine(96, 80, 6,") and "n_probes=2" in beam[0] and "n_frames=0" in beam[0] and "frame_batch=1" in beam[0]
    assert result[0].startswith("Engine(48, 40, 1,") and "n_probes=2" in result[0] and "n_frames=1" in result[0] and "frame_batch=1" in result[0]
    assert beam[1:] == ["set_kirkland(f8(103,3,4))", "set_slices(f8(6,), f8(6,))", "set_aberrations(None)", "smatrix_begin((2,2), 30)"] + 2 * [
        "build_potential(f8(10,3), i4(10,), 2)", "smatrix_build()",
        "smatrix_probes_cropped(LoggedEngine, xy[0,1], 0)", "smatrix_probes_cropped(LoggedEngine, xy[2,3], 0)",
        "smatrix_probes_cropped(LoggedEngine, xy[4,4], 0)"]
    assert result[1:] == ["set_detectors(u2(1920,), (intensity), f4(48,), f4(40,))"] + 2 * ["detect(0, 1, B=2)", "detect(0, 1, B=2)", "detect(0, 1, B=1)"]
    assert all(c[1][0] is calc._engine for c in calc._beam_engine.calls if c[0] == "smatrix_probes_cropped")
    # the two engines interleave: every synthesis is followed by its reduction
    loop = [c for c in LoggedEngine.log if c[1] in ("smatrix_build", "smatrix_probes_cropped", "detect")]
    assert loop == 2 * ([("beam", "smatrix_build")] + 3 * [("beam", "smatrix_probes_cropped"), ("result", "detect")])
    assert calc.probe_batch == 2 and out.prism_crop == (2, 2)
    assert len(out.kxs) == 48 and len(out.kys) == 40
    kx_full = np.fft.fftshift(np.fft.fftfreq(96, calc.sampling)).astype(np.float32)
    assert np.allclose(np.asarray(out.kxs), kx_full[prism.crop_index(96, 2)], rtol=1e-6, atol=0)


def test_call_order_of_cropped_run_diffraction_and_polar(traj, monkeypatch):
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.polar_data import PolarDetector
    calc, wf, (beam, result) = _recorded(monkeypatch, traj, "run", prism=Prism((2, 4), crop=True), k_window=(24, 20), k_bin=(2, 2))
    Bm = len(prism.beams(96, 80, calc.dx, calc.dy, 30.0, LAM, (2, 4)))
    assert calc._prism_Bm == Bm and Bm < 5 * 8
    assert beam[0].startswith("Engine(96, 80, 6,") and f"n_probes={min(5, Bm)}" in beam[0] and "n_frames=0" in beam[0]
    assert "window=None" in beam[0] and "k_bin" not in beam[0].replace("k_bin=None", "")
    assert result[0].startswith("Engine(48, 20, 1,") and "n_probes=5" in result[0] and "n_frames=2" in result[0]
    assert "window=(24,20)" in result[0] and "k_bin=(2,2)" in result[0]
    per_frame = ["build_potential(f8(10,3), i4(10,), 2)", "smatrix_build()"]
    assert beam[4:] == ["smatrix_begin((2,4), 30)"] + per_frame + ["smatrix_probes_cropped(LoggedEngine, xy[0,1,2,3,4], 0)"] + per_frame + [
        "smatrix_probes_cropped(LoggedEngine, xy[0,1,2,3,4], 1)"]
    assert not any(l.startswith(("set_probes", "smatrix_probes(")) for l in beam + result)
    assert [l.split("(")[0] for l in result[1:]] == ["synchronize", "wavefunction_c128"]
    assert wf.prism_crop == (2, 4) and wf._engine is calc._engine and len(wf.kxs) == 12 and len(wf.kys) == 10

    calc, out, (beam, result) = _recorded(monkeypatch, traj, "run_diffraction", diffraction=Diffraction(bin=(2, 2)), detectors=_adf(),
                                          probe_batch=4, prism=Prism(2, crop=True))
    assert [l for l in beam if l.startswith(("smatrix", "build"))] == ["smatrix_begin((2,2), 30)"] + 2 * [
        "build_potential(f8(10,3), i4(10,), 2)", "smatrix_build()", "smatrix_probes_cropped(LoggedEngine, xy[0,1,2,3], 0)",
        "smatrix_probes_cropped(LoggedEngine, xy[4,4,4,4], 0)"]
    assert result[2:] == 2 * ["diffract(0, 1, B=4, bin=(2,2))", "detect(0, 1, B=4)", "diffract(0, 1, B=1, bin=(2,2))", "detect(0, 1, B=1)"]
    assert out.intensity.shape == (5, 24, 20) and out.prism_crop == (2, 2) and out.stem.prism_crop == (2, 2)

    calc, out, (beam, result) = _recorded(monkeypatch, traj, "run_polar", polar=PolarDetector(inner=0.0, outer=120.0, step=30.0, n_azimuthal=2),
                                          probe_batch=4, prism=Prism(2, crop=True))
    assert result[1].startswith("set_polar(") and [l.split("(")[0] for l in result[2:]] == 4 * ["polar_detect"]
    assert not any(l.startswith(("polar_detect", "set_polar", "detect", "diffract")) for l in beam)
    assert out.prism_crop == (2, 2) and len(out.kxs) == 48


def test_crop_at_interpolation_one_runs_uncropped(traj, monkeypatch):
    calc, out, engines = _recorded(monkeypatch, traj, "run_detectors", detectors=_adf(), probe_batch=2, prism=Prism(1, crop=True))
    assert len(engines) == 1 and calc._beam_engine is None and calc._crop is None
    assert engines[0][0].startswith("Engine(96, 80, 6,") and any(l.startswith("smatrix_probes(") for l in engines[0])
    assert not hasattr(out, "prism_crop")
    _, out, engines = _recorded(monkeypatch, traj, "run_detectors", detectors=_adf(), probe_batch=2, prism=Prism(2))
    assert len(engines) == 1 and not hasattr(out, "prism_crop")


def test_validation_against_the_cropped_grid(traj, monkeypatch):
    from pyslice_amd import _native
    from pyslice_amd.diffraction_data import Diffraction

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(_native, "Engine", no_engine)
    kw = dict(aperture=30.0, voltage_eV=EV, probe_positions=PP)
    # 96 x 80 holds these, the cropped 48 x 40 does not
    with pytest.raises(ValueError, match="cropped 48 x 40"):
        _calc(prism=Prism(2, crop=True), k_window=(64, 40)).setup(traj, **kw)
    with pytest.raises(ValueError, match="cropped 48 x 40"):
        _calc(prism=Prism(2, crop=True), detectors=_adf(), k_window=(48, 42)).setup(traj, **kw)
    with pytest.raises(ValueError, match="48 x 40 is not a multiple of k_bin"):
        _calc(prism=Prism(2, crop=True), k_bin=(32, 1)).setup(traj, **kw)
    with pytest.raises(ValueError, match="48 x 40 is not a multiple of the diffraction bin"):
        _calc(prism=Prism(2, crop=True), diffraction=Diffraction(bin=(32, 1))).setup(traj, **kw)
    # every refusal of prism stays
    with pytest.raises(ValueError, match="aperture"):
        _calc(prism=Prism(2, crop=True), detectors=_adf()).setup(traj, aperture=0.0, voltage_eV=EV, probe_positions=PP)
    with pytest.raises(ValueError, match="suggest_sampling"):
        _calc(prism=Prism(7, crop=True)).setup(traj, **kw)
    for bad in [dict(diffraction=Diffraction(bin=(2, 2), split=True)), dict(layers=[1]), dict(stream_tile=2), dict(cache=True)]:
        with pytest.raises((ValueError, NotImplementedError), match="not built"):
            _calc(prism=Prism(2, crop=True), **bad)
    # and the uncropped run takes the same arguments (the recording engine stands in for the device)
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    _calc(prism=Prism(2), k_window=(64, 40)).setup(traj, **kw)
    _calc(prism=Prism(2), k_bin=(32, 1)).setup(traj, **kw)
    _calc(prism=Prism(2, crop=True), k_window=(48, 40)).setup(traj, **kw)


def test_fit_probe_batch_is_larger_with_crop(traj, monkeypatch):
    """per probe 32 * gx * gy + 8 * pitch bytes on the cropped grid; S, the stacks and the build chunk of min(Pc, Bm) beams on the full"""
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    full = _calc(detectors=_adf(), prism=Prism(2))
    full.setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    crop = _calc(detectors=_adf(), prism=Prism(2, crop=True))
    crop.setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    Bm = full._prism_Bm
    assert Bm == crop._prism_Bm == 41
    fixed = 16.0 * 6 * 96 * 80 + full._phase_table_bytes(1) + 8.0 * Bm * 96 * 80 + 1e9
    per_full = 32.0 * 96 * 80 + 8.0 * 7680
    per_crop = 32.0 * 48 * 40 + 8.0 * 1920
    assert per_full == 4 * per_crop
    free_b = (fixed + 100 * per_full) / 0.9                                   # room for 100 full-grid probes: 64 of 256, 128 of 128 ...
    assert full._fit_probe_batch(free_b, 256, 1) == 64
    # ... and for 256 cropped probes next to the chunk of Bm beams
    assert 256 * per_crop + Bm * 32.0 * 96 * 80 < 100 * per_full
    assert crop._fit_probe_batch(free_b, 256, 1) == 256
    free_b = (fixed + 8 * per_full + 1.0) / 0.9                               # a tight device: the chunk shrinks with the batch
    assert full._fit_probe_batch(free_b, 256, 1) == 8
    got = crop._fit_probe_batch(free_b, 256, 1)
    assert got * (per_crop + 32.0 * 96 * 80) <= 8 * per_full + 1.0 < 2 * got * (per_crop + 32.0 * 96 * 80)


def test_entry_point_in_the_header_and_binding():
    import re
    from pyslice_amd import _native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mslice.h")).read()
    assert "msl_smatrix_probes_cropped" in _native.EXPORTS
    assert re.search(r"int\s+msl_smatrix_probes_cropped\(msl_handle\* src, msl_handle\* dst, const double\* xy, int32_t n_probes, int32_t slot\);", hdr)
    assert callable(_native.Engine.smatrix_probes_cropped)
