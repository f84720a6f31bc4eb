"""PRISM on the host: the beam list, the window, the float64 definition against the oracle, the refusals and the engine call order."""
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
# (nx, ny, mrad, f, Bm) at 100 kV, 0.1 A pixels
BEAM_COUNTS = [(96, 80, 30.0, (1, 1), 155), (96, 80, 30.0, (2, 2), 41), (96, 80, 30.0, (2, 1), 79), (45, 63, 40.0, (1, 1), 101),
               (45, 63, 40.0, (3, 3), 11), (128, 128, 30.0, (2, 2), 89), (128, 128, 30.0, (4, 4), 21)]
POSITIONS = [(1.3, 2.05), (4.8, 0.4), (0.0, 0.0)]


def _axes(nx, ny, nz=1):
    return np.arange(nx) * 0.1, np.arange(ny) * 0.1, np.arange(nz) * 0.5


@pytest.mark.parametrize("nx,ny,mrad,f,count", BEAM_COUNTS)
def test_beams_equal_brute_force_and_the_table(nx, ny, mrad, f, count):
    got = prism.beams(nx, ny, 0.1, 0.1, mrad, LAM, f)
    want = []
    for mx in range(nx):
        hx = mx if mx < (nx + 1) // 2 else mx - nx
        for my in range(ny):
            hy = my if my < (ny + 1) // 2 else my - ny
            if hx % f[0] == 0 and hy % f[1] == 0 and np.sqrt((hx / (nx * 0.1)) ** 2 + (hy / (ny * 0.1)) ** 2) < mrad * 1e-3 / LAM:
                want.append((hx, hy))
    assert got.dtype == np.int32 and got.tolist() == [list(b) for b in want]
    assert len(got) == count


def test_beams_refusals():
    for bad in [dict(mrad=0.0), dict(mrad=-1.0), dict(f=(0, 1)), dict(f=(5, 1)), dict(f=(1, 3))]:
        kw = dict(mrad=30.0, f=(1, 1))
        kw.update(bad)
        with pytest.raises(ValueError):
            prism.beams(96, 80, 0.1, 0.1, kw["mrad"], LAM, kw["f"])


@pytest.mark.parametrize("nx,ny,mrad", [(96, 80, 30.0), (45, 63, 40.0)])
def test_window_centre_is_where_the_probe_peaks(nx, ny, mrad):
    xs, ys, _ = _axes(nx, ny)
    probes = orc.batched_probes(orc.probe_array(xs, ys, mrad, EV), xs, ys, POSITIONS)
    for p, (px, py) in zip(probes, POSITIONS):
        a = np.abs(p)
        ix, iy = np.unravel_index(np.argmax(a), a.shape)
        cx, cy = prism.window_centre(nx, 0.1, px), prism.window_centre(ny, 0.1, py)
        if py == 2.05:
            # 2.05 / 0.1 is half a pixel: the probe sits between two pixels whose moduli differ by rounding only, and argmax
            # names one of the pair -- the centre must be one of the two and attain the maximum
            assert cx == ix and cy in ((-(ny // 2) - 20) % ny, (-(ny // 2) - 21) % ny) and abs(iy - cy) <= 1
            assert a[cx, cy] >= a.max() * (1 - 1e-12)
        else:
            assert (cx, cy) == (ix, iy)


def test_window_mask_wraps_and_counts():
    for n, f, p in [(96, 2, 0.0), (96, 2, 4.8), (45, 3, 1.3), (63, 3, 2.05), (80, 1, 0.4)]:
        m = prism.window_mask(n, 0.1, p, f)
        assert m.sum() == n // f and m[prism.window_centre(n, 0.1, p)]


@pytest.fixture(scope="module")
def small_cell():
    nx, ny, nz = 45, 63, 4
    xs, ys, zs = _axes(nx, ny, nz)
    rng = np.random.default_rng(3)
    n_atoms = int(round(0.05 * nx * 0.1 * ny * 0.1 * nz * 0.5))
    pos = rng.random((n_atoms, 3)) * np.array([nx * 0.1, ny * 0.1, nz * 0.5])
    V = orc.potential(xs, ys, zs, pos, np.full(n_atoms, 79))
    hb = prism.beams(nx, ny, 0.1, 0.1, 40.0, LAM)
    S = orc.propagate(prism.plane_waves(nx, ny, hb), V, xs, ys, zs, EV)
    return xs, ys, zs, V, hb, S


def test_prism_waves_at_f1_is_the_multislice_exit_wave(small_cell):
    xs, ys, zs, V, hb, S = small_cell
    want = orc.propagate(orc.batched_probes(orc.probe_array(xs, ys, 40.0, EV), xs, ys, POSITIONS), V, xs, ys, zs, EV)
    got = prism.prism_waves(S, hb, POSITIONS, 0.1, 0.1)
    for g, w in zip(got, want):
        assert np.linalg.norm(g - w) / np.linalg.norm(w) < 1e-12


def test_prism_waves_at_f1_with_aberrations(small_cell):
    """the coefficient carries exp(-i chi): the aberrated probe of the project's own definition, ifft2(mask ramp exp(-i chi))"""
    from pyslice_amd.aberrations import Aberrations
    xs, ys, zs, V, hb, S = small_cell
    ab = Aberrations(defocus=150.0, Cs=2e5, astigmatism=40.0, astigmatism_angle=0.7)
    nx, ny = len(xs), len(ys)
    kx, ky = np.fft.fftfreq(nx, 0.1), np.fft.fftfreq(ny, 0.1)
    base_k = np.fft.fft2(orc.probe_array(xs, ys, 40.0, EV)) * np.exp(-1j * ab.chi(kx[:, None], ky[None, :], LAM))
    probes = orc.batched_probes(np.fft.ifft2(base_k), xs, ys, POSITIONS)
    want = orc.propagate(probes, V, xs, ys, zs, EV)
    got = prism.prism_waves(S, hb, POSITIONS, 0.1, 0.1, wavelength=LAM, aberrations=ab)
    for g, w in zip(got, want):
        assert np.linalg.norm(g - w) / np.linalg.norm(w) < 1e-12


def test_prism_waves_window_is_zero_outside_and_scaled_inside(small_cell):
    xs, ys, zs, V, hb, S = small_cell
    hb3 = prism.beams(45, 63, 0.1, 0.1, 40.0, LAM, (3, 3))
    keep = [i for i, b in enumerate(hb.tolist()) if b in hb3.tolist()]
    got = prism.prism_waves(S[keep], hb3, POSITIONS, 0.1, 0.1, (3, 3))
    for g, (px, py) in zip(got, POSITIONS):
        w = prism.window_mask(45, 0.1, px, 3)[:, None] & prism.window_mask(63, 0.1, py, 3)[None, :]
        assert w.sum() == 15 * 21 and not g[~w].any() and np.abs(g[w]).min() > 0


@pytest.mark.parametrize("bad", [0, -1, (1,), (1, 2, 3), (0, 1), 1.5, (2, 1.0), "2", True, None])
def test_prism_refuses_bad_interpolations(bad):
    with pytest.raises(ValueError):
        Prism(bad)


def test_prism_accepts_an_integer_or_a_pair():
    assert Prism().interpolation == (1, 1) and Prism(2).interpolation == (2, 2) and Prism((2, 1)).interpolation == (2, 1)
    assert Prism(np.int64(4)).interpolation == (4, 4)


# ---- the calculator ---------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (4.8, 0.4), (0.0, 0.0), (2.5, 2.5), (3.1, 0.9)]


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


def test_constructor_refusals_say_not_built():
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.imaging import Imaging
    with pytest.raises(ValueError):
        _calc(prism=2)
    for kw in [dict(diffraction=Diffraction(bin=(2, 2), split=True)), dict(imaging=Imaging()), dict(layers=[1]), dict(stream_tile=2),
               dict(cache=True)]:
        with pytest.raises((ValueError, NotImplementedError), match="not built"):
            _calc(prism=Prism(1), **kw)


def test_setup_refusals_before_device_work(traj, monkeypatch):
    from pyslice_amd import _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(_native, "Engine", no_engine)
    with pytest.raises(ValueError, match="aperture"):
        _calc(prism=Prism(1), detectors=_adf()).setup(traj, aperture=0.0, voltage_eV=EV, probe_positions=PP)
    with pytest.raises(ValueError, match="suggest_sampling"):
        _calc(prism=Prism(7), detectors=_adf()).setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    with pytest.raises(ValueError, match="suggest_sampling"):
        _calc(prism=Prism((1, 3))).setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="not built"):
        _calc(prism=Prism(1)).setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)


def _recorded(monkeypatch, traj, run, **kw):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    calc = _calc(**kw)
    calc.setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    getattr(calc, run)()
    eng = calc._engine
    return calc, format_calls([eng.created] + eng.calls, PP)


MULTISLICE_DETECTORS = [
    "set_kirkland(f8(103,3,4))", "set_slices(f8(6,), f8(6,))", "set_aberrations(None)", "set_detectors(u2(7680,), (intensity), f4(96,), f4(80,))",
    "build_potentials(f8(2,10,3), i4(10,), 2)",
    "set_probes(30, xy[0,1])", "propagate_frames(0, 2)", "detect(0, 2, B=2)",
    "set_probes(30, xy[2,3])", "propagate_frames(0, 2)", "detect(0, 2, B=2)",
    "set_probes(30, xy[4,4])", "propagate_frames(0, 2)", "detect(0, 2, B=1)"]

PRISM_DETECTORS = [
    "set_kirkland(f8(103,3,4))", "set_slices(f8(6,), f8(6,))", "set_aberrations(None)", "set_detectors(u2(7680,), (intensity), f4(96,), f4(80,))",
    "smatrix_begin((1,1), 30)"] + 2 * [
    "build_potential(f8(10,3), i4(10,), 2)", "smatrix_build()",
    "smatrix_probes(xy[0,1], 0)", "detect(0, 1, B=2)",
    "smatrix_probes(xy[2,3], 0)", "detect(0, 1, B=2)",
    "smatrix_probes(xy[4,4], 0)", "detect(0, 1, B=1)"]


def test_call_order_of_a_prism_detector_run(traj, monkeypatch):
    """2 frames, 5 probes, probe_batch = 2: per frame one potential and one S-matrix, then three probe batches into slot 0"""
    calc, lines = _recorded(monkeypatch, traj, "run_detectors", detectors=_adf(), probe_batch=2, prism=Prism(1))
    assert "frame_batch=1" in lines[0] and "n_probes=2" in lines[0] and "n_frames=1" in lines[0]
    assert lines[1:] == PRISM_DETECTORS
    assert calc._prism_Bm == len(prism.beams(96, 80, calc.dx, calc.dy, 30.0, LAM))


def test_call_order_without_prism_is_unchanged(traj, monkeypatch):
    calc, lines = _recorded(monkeypatch, traj, "run_detectors", detectors=_adf(), probe_batch=2)
    assert "frame_batch=2" in lines[0] and "n_probes=2" in lines[0] and "n_frames=2" in lines[0]
    assert lines[1:] == MULTISLICE_DETECTORS


def test_call_order_of_prism_run_and_diffraction(traj, monkeypatch):
    from pyslice_amd.diffraction_data import Diffraction
    calc, lines = _recorded(monkeypatch, traj, "run", prism=Prism((2, 2)), k_window=(48, 40))
    assert "frame_batch=1" in lines[0] and "n_probes=5" in lines[0] and "n_frames=2" in lines[0]
    per_frame = ["build_potential(f8(10,3), i4(10,), 2)", "smatrix_build()"]
    assert lines[4:-2] == ["smatrix_begin((2,2), 30)"] + per_frame + ["smatrix_probes(xy[0,1,2,3,4], 0)"] + per_frame + ["smatrix_probes(xy[0,1,2,3,4], 1)"]
    assert not any(l.startswith("set_probes") for l in lines)
    calc, lines = _recorded(monkeypatch, traj, "run_diffraction", diffraction=Diffraction(bin=(2, 2)), probe_batch=4, prism=Prism(2))
    assert [l for l in lines if l.startswith(("smatrix", "diffract", "build"))] == ["smatrix_begin((2,2), 30)"] + 2 * [
        "build_potential(f8(10,3), i4(10,), 2)", "smatrix_build()", "smatrix_probes(xy[0,1,2,3], 0)", "diffract(0, 1, B=4, bin=(2,2))",
        "smatrix_probes(xy[4,4,4,4], 0)", "diffract(0, 1, B=1, bin=(2,2))"]


def test_fit_probe_batch_counts_the_s_matrix(traj, monkeypatch):
    """8 * Bm * nx * ny bytes of S join what the probe batch must leave room for"""
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    calc = _calc(detectors=_adf(), prism=Prism(1))
    calc.setup(traj, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    S_bytes = 8.0 * calc._prism_Bm * 96 * 80
    assert calc._prism_Bm > 100
    per_probe = 32.0 * 96 * 80 + 8.0 * 7680
    fixed = 16.0 * 6 * 96 * 80 + calc._phase_table_bytes(1) + 1e9
    free_b = (fixed + S_bytes + 8 * per_probe + 1.0) / 0.9            # room for 8 probes next to S, not for 16
    assert calc._fit_probe_batch(free_b, 16, 1) == 8
    calc._prism_Bm = 0
    assert calc._fit_probe_batch(free_b, 16, 1) == 16


def test_entry_points_in_the_header_and_binding():
    import re
    from pyslice_amd import _native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mslice.h")).read()
    assert re.search(r"MSL_BUF_SMATRIX\s*=\s*12\b", hdr) and _native.BUF_SMATRIX == 12
    assert re.search(r"#define MSL_ABI_VERSION 3\b", hdr)
    for name in ("msl_smatrix_begin", "msl_smatrix_beams", "msl_smatrix_build", "msl_smatrix_probes", "msl_smatrix_end"):
        assert name in _native.EXPORTS and re.search(r"\b" + name + r"\(", hdr)
    for name in ("smatrix_begin", "smatrix_beams", "smatrix_build", "smatrix_probes", "smatrix_end"):
        assert callable(getattr(_native.Engine, name))
