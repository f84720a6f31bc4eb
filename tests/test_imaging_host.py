"""HRTEM imaging on the host: the Imaging request and its NumPy transfer function, ImageData, the refusals of the calculator, the ABI
entries, and the engine calls of run_images() on an engine that only records them."""
import math
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.0370143628314            # 100 keV


# ------------------------------------------------------------------ 1. the ABI
def test_image_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name in ("msl_image_reset", "msl_image_add", "msl_image_download"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr)
    assert _native.ABI_VERSION == 3
    for meth in ("image_reset", "image_add", "image_download"):
        assert callable(getattr(_native.Engine, meth))


# ------------------------------------------------------------------ 2. the request
@pytest.mark.parametrize("kw", [dict(aberrations="Cs"), dict(aperture_mrad=float("nan")), dict(aperture_mrad=0.0), dict(aperture_mrad=-3.0),
                                dict(aperture_mrad="wide"), dict(defocus_series=()), dict(defocus_series=[0.0, float("inf")]),
                                dict(defocus_series=["a"]), dict(focal_spread=float("nan")), dict(focal_spread=-1.0),
                                dict(focal_points=2, focal_spread=10.0), dict(focal_points=0), dict(focal_points=-3), dict(focal_points=3.0, focal_spread=10.0),
                                dict(focal_points=True), dict(focal_points=3), dict(focal_points=5, focal_spread=0.0)])
def test_imaging_validation(kw):
    from pyslice_amd import Imaging
    with pytest.raises(ValueError, match="Imaging"):
        Imaging(**kw)


def test_imaging_defaults_and_frozen():
    from dataclasses import FrozenInstanceError
    from pyslice_amd import Aberrations, Imaging
    im = Imaging()
    assert im.aberrations is None and im.aperture_mrad is None and im.defocus_series == (0.0,) and im.focal_spread == 0.0 and im.focal_points == 1
    assert np.array_equal(im.polar(), np.zeros((14, 2)))
    assert im.aperture_k(LAM) == 0.0
    im = Imaging(aberrations=Aberrations(Cs=1.2e7), aperture_mrad=12, defocus_series=np.array([-100, 0, 50]), focal_spread=30, focal_points=np.int64(3))
    assert im.defocus_series == (-100.0, 0.0, 50.0) and isinstance(im.focal_points, int) and im.aperture_mrad == 12.0
    assert im.aperture_k(LAM) == (12.0 * 1e-3) / LAM
    assert Imaging(defocus_series=25.0).defocus_series == (25.0,)
    with pytest.raises(FrozenInstanceError):
        im.focal_spread = 1.0


def test_nodes():
    from pyslice_amd import Imaging
    for im in (Imaging(), Imaging(focal_spread=40.0), Imaging(focal_spread=40.0, focal_points=1)):
        d, w = im.nodes()
        assert d.tolist() == [0.0] and w.tolist() == [1.0]                     # exactly
    for N in (3, 5, 9, 21):
        d, w = Imaging(focal_spread=40.0, focal_points=N).nodes()
        x, om = np.polynomial.hermite.hermgauss(N)
        assert d.shape == w.shape == (N,)
        assert abs(w.sum() - 1.0) <= 1e-15
        assert np.array_equal(d, math.sqrt(2.0) * 40.0 * x) and np.array_equal(w, om / math.sqrt(math.pi))
        assert d[N // 2] == 0.0 and np.allclose(d, -d[::-1], rtol=0, atol=1e-12)
        assert abs((w * d * d).sum() - 40.0 ** 2) <= 1e-9 * 40.0 ** 2           # the variance of the Gaussian


def test_polar_adds_defocus_and_node_to_C10():
    from pyslice_amd import Aberrations, Imaging
    ab = Aberrations(C10=-300.0, C12=20.0, phi12=0.4, Cs=1.0e7)
    im = Imaging(aberrations=ab, defocus_series=(-50.0, 0.0, 120.0), focal_spread=25.0, focal_points=3)
    d, _ = im.nodes()
    for f in range(3):
        for i in range(3):
            p = im.polar(f, i)
            want = ab.as_polar()
            want[0, 0] = -300.0 + im.defocus_series[f] + d[i]
            assert p.shape == (14, 2) and p.dtype == np.float64 and np.array_equal(p, want)
    assert np.array_equal(ab.as_polar()[0], [-300.0, 0.0])                      # the request is left as it is


def test_transfer_is_exp_minus_i_chi_inside_a_strict_aperture():
    from pyslice_amd import Aberrations, Imaging
    nx, ny, d = 48, 40, 0.1
    kx, ky = np.fft.fftfreq(nx, d)[:, None], np.fft.fftfreq(ny, d)[None, :]
    ab = Aberrations(C10=-200.0, Cs=1.3e7, C12=30.0, phi12=0.7, C21=500.0, phi21=-1.1)
    # an aperture radius that IS the |k| of a pixel: that pixel and its ring are outside (strict <)
    k_edge = float(np.hypot(kx[5, 0], ky[0, 3]))
    mrad = k_edge * LAM * 1e3
    im = Imaging(aberrations=ab, aperture_mrad=mrad, defocus_series=(0.0, 80.0), focal_spread=20.0, focal_points=3)
    k_ap = im.aperture_k(LAM)
    r = np.sqrt(kx * kx + ky * ky)
    inside = r < k_ap
    assert 10 < inside.sum() < nx * ny
    H = im.transfer(kx, ky, LAM, f=0, i=1)                                      # the centre node: delta = 0
    assert H.shape == (nx, ny) and H.dtype == np.complex128
    assert np.array_equal(H[~inside], np.zeros((~inside).sum()))
    assert np.array_equal(H[inside], np.exp(-1j * ab.chi(kx, ky, LAM))[inside])
    assert np.allclose(np.abs(H[inside]), 1.0, rtol=0, atol=1e-15)
    # defocus_series[f] and the node add to C10
    dl, _ = im.nodes()
    for f, i in ((1, 0), (1, 2), (0, 0), (1, 1)):
        ab2 = Aberrations(C10=-200.0 + im.defocus_series[f] + dl[i], Cs=1.3e7, C12=30.0, phi12=0.7, C21=500.0, phi21=-1.1)
        assert np.array_equal(im.transfer(kx, ky, LAM, f=f, i=i)[inside], np.exp(-1j * ab2.chi(kx, ky, LAM))[inside])
    # no aberrations, no aperture: ones everywhere; defocus alone is the Fresnel factor exp(-i pi lambda dz k^2)
    assert np.array_equal(Imaging().transfer(kx, ky, LAM), np.ones((nx, ny), dtype=np.complex128))
    Hd = Imaging(defocus_series=(37.0,)).transfer(kx, ky, LAM)
    assert np.allclose(Hd, np.exp(-1j * np.pi * LAM * 37.0 * r * r), rtol=0, atol=1e-12)


# ------------------------------------------------------------------ 3. ImageData
def test_image_data_accessors():
    from pyslice_amd import ImageData, Imaging
    rng = np.random.default_rng(3)
    I = rng.random((3, 2, 4, 12, 10))
    im = Imaging(defocus_series=(-10.0, 0.0, 10.0, 20.0))
    d = ImageData(intensity=I, xs=np.arange(12) * 0.1, ys=np.arange(10) * 0.1, defocus=im.defocus_series, layer=[4, 9], n_frames=5,
                  probe_positions=[(0, 0), (1, 1), (2, 2)], imaging=im)
    assert d.intensity.shape == (3, 2, 4, 12, 10) and d.intensity.dtype == np.float64
    assert d.defocus.shape == (4,) and d.layer.tolist() == [4, 9] and d.n_frames == 5 and d.imaging is im
    assert np.array_equal(d.image(), I[0, -1, 0]) and np.array_equal(d.image(2, 0, 1), I[1, 0, 2])
    assert np.array_equal(d.image(defocus_index=3, layer=1, probe=2), I[2, 1, 3])
    img = I[1, 0, 2]
    want = np.abs(np.fft.fftshift(np.fft.fft2(img - img.mean()))) ** 2
    g = d.diffractogram(2, 0, 1)
    assert g.shape == (12, 10) and np.array_equal(g, want)
    assert g[6, 5] <= 1e-20 * want.max()                                        # the mean is gone: nothing at k = 0
    with pytest.raises(ValueError, match="shape"):
        ImageData(intensity=I[:, :1], xs=np.arange(12), ys=np.arange(10), defocus=im.defocus_series, layer=[4, 9], n_frames=5,
                  probe_positions=None, imaging=im)
    with pytest.raises(ValueError, match="shape"):
        ImageData(intensity=I[0], xs=np.arange(12), ys=np.arange(10), defocus=im.defocus_series, layer=[4, 9], n_frames=5,
                  probe_positions=None, imaging=im)


# ------------------------------------------------------------------ 4. refusals of the calculator
def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def test_constructor_refusals():
    from pyslice_amd import Detector, Diffraction, Imaging
    from pyslice_amd.calculators import MultisliceCalculator
    im = Imaging()
    for what, kw in (("k_window", dict(k_window=(16, 16))), ("k_bin", dict(k_bin=(2, 2))), ("cache", dict(cache=True)),
                     ("stream_tile", dict(stream_tile=4)), ("detectors", dict(detectors=[Detector("bf", outer=20.0)])),
                     ("diffraction", dict(diffraction=Diffraction()))):
        with pytest.raises(ValueError, match=f"imaging cannot be combined with {what}"):
            MultisliceCalculator(progress=False, imaging=im, **kw)
    with pytest.raises(ValueError, match="imaging of thickness-series layers is not built"):
        MultisliceCalculator(progress=False, imaging=im, layers=[1])
    with pytest.raises(ValueError, match="Imaging object"):
        MultisliceCalculator(progress=False, imaging=dict(defocus=1.0))
    MultisliceCalculator(progress=False, imaging=im, probe_batch=2)               # probe_batch applies to imaging runs
    with pytest.raises(ValueError, match="probe_batch"):
        MultisliceCalculator(progress=False, probe_batch=2)


def test_run_names_run_images_and_run_images_needs_the_mode(monkeypatch):
    from pyslice_amd import Imaging, _native
    from pyslice_amd.calculators import MultisliceCalculator
    with pytest.raises(RuntimeError, match="run_images"):
        MultisliceCalculator(progress=False, imaging=Imaging()).run()
    with pytest.raises(RuntimeError, match="setup"):
        MultisliceCalculator(progress=False, imaging=Imaging()).run_images()
    with pytest.raises(RuntimeError, match="imaging=Imaging"):
        MultisliceCalculator(progress=False).run_images()


def test_several_ranks_refused_before_device_work(monkeypatch):
    from pyslice_amd import Imaging, _native, distributed
    from pyslice_amd.calculators import MultisliceCalculator
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))

    def no_engine(*a, **k):
        raise AssertionError("the refusal must come before any device work")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = MultisliceCalculator(progress=False, imaging=Imaging())
    with pytest.raises(NotImplementedError, match="imaging: runs over several ranks are not supported"):
        calc.setup(_trajectory(2), aperture=0.0, voltage_eV=100e3)


# ------------------------------------------------------------------ 5. the engine calls of run_images()
class ImagingEngine(RecordingEngine):
    """the recorder, answering image_download with images that are 10 everywhere"""

    def image_download(self, first, n):
        self.calls.append(("image_download", (first, n), {}))
        return np.full((n, self.wx, self.wy), 10.0)


def _run(monkeypatch, imaging, n_frames, positions, **kw):
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", ImagingEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    calc = calculators.MultisliceCalculator(progress=False, imaging=imaging, **kw)
    calc.setup(_trajectory(n_frames), aperture=0.0, voltage_eV=100e3, probe_positions=positions)
    data = calc.run_images()
    eng = calc._engine
    # (the recorder's formatter takes any (n, 2) array for probe positions: the polar coefficients go in as their dtype and shape)
    calls = [(name, a, {key: (f"f8{v.shape}".replace(" ", "") if key == "polar" else v) for key, v in k.items()}) for name, a, k in eng.calls]
    return data, eng.created[2], format_calls(calls, positions)


def test_run_images_call_order_one_probe(monkeypatch):
    """P = 1, T = 5, frame_batch = 2, F = 2, N = 3: per frame batch one image_add per (defocus, node), f outside, i inside"""
    from pyslice_amd import Aberrations, Imaging
    im = Imaging(aberrations=Aberrations(Cs=1.0e7), aperture_mrad=20.0, defocus_series=(-100.0, 50.0), focal_spread=30.0, focal_points=3)
    data, created, lines = _run(monkeypatch, im, 5, [(1.0, 1.5)], frame_batch=2)
    assert (created["n_probes"], created["n_frames"], created["frame_batch"], created["window"], created["k_bin"]) == (1, 2, 2, None, None)
    k = f"{0.02 / LAM:.12g}"
    w = ["0.166666666667", "0.666666666667", "0.166666666667"]

    def adds(n):
        return [f"image_add(0, {n}, polar=f8(14,2), aperture_k={k}, weight={w[i]}, first={f}, stride=2, B=1)" for f in range(2) for i in range(3)]
    assert lines == (["set_kirkland(f8(103,3,4))", "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(0, xy[0])",
                      "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "image_reset(2)"] + adds(2)
                     + ["build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)"] + adds(2)
                     + ["build_potentials(f8(1,2,3), i4(2,), 2)", "propagate_frames(0, 1)"] + adds(1)
                     + ["image_download(0, 2)"])
    # the division by T, and the result's fields
    assert data.intensity.shape == (1, 1, 2, 32, 32) and np.array_equal(data.intensity, np.full((1, 1, 2, 32, 32), 2.0))
    assert data.n_frames == 5 and data.defocus.tolist() == [-100.0, 50.0] and data.layer.tolist() == [2] and data.imaging is im
    assert len(data.xs) == 32 and len(data.ys) == 32 and data.probe_positions == [(1.0, 1.5)]


def test_run_images_polar_of_every_add(monkeypatch):
    from pyslice_amd import Aberrations, Imaging, _native, calculators
    im = Imaging(aberrations=Aberrations(Cs=1.0e7, C10=-40.0), defocus_series=(-100.0, 50.0), focal_spread=30.0, focal_points=3)
    monkeypatch.setattr(_native, "Engine", ImagingEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    calc = calculators.MultisliceCalculator(progress=False, imaging=im, frame_batch=5)
    calc.setup(_trajectory(5), aperture=0.0, voltage_eV=100e3)
    calc.run_images()
    adds = [c for c in calc._engine.calls if c[0] == "image_add"]
    assert len(adds) == 6
    d, w = im.nodes()
    for (name, a, kw), (f, i) in zip(adds, [(f, i) for f in range(2) for i in range(3)]):
        assert kw["polar"][0, 0] == -40.0 + im.defocus_series[f] + d[i] and kw["polar"][4, 0] == 1.0e7
        assert kw["weight"] == w[i] and kw["aperture_k"] == 0.0


def test_run_images_call_order_two_probe_batches(monkeypatch):
    """P = 2, probe_batch = 1, T = 3, frame_batch = 2: probe batches outside, the accumulator reset for each, the potentials of every
    frame built once per probe batch"""
    from pyslice_amd import Imaging
    pp = [(1.0, 1.5), (2.0, 0.5)]
    data, created, lines = _run(monkeypatch, Imaging(), 3, pp, frame_batch=2, probe_batch=1)
    assert (created["n_probes"], created["n_frames"], created["frame_batch"]) == (1, 2, 2)

    def batch(p):
        return [f"set_probes(0, xy[{p}])", "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "image_reset(1)",
                "image_add(0, 2, polar=f8(14,2), aperture_k=0, weight=1, first=0, stride=1, B=1)",
                "build_potentials(f8(1,2,3), i4(2,), 2)", "propagate_frames(0, 1)",
                "image_add(0, 1, polar=f8(14,2), aperture_k=0, weight=1, first=0, stride=1, B=1)", "image_download(0, 1)"]
    assert lines == ["set_kirkland(f8(103,3,4))", "set_slices(f8(3,), f8(3,))", "set_aberrations(None)"] + batch(0) + batch(1)
    assert data.intensity.shape == (2, 1, 1, 32, 32) and np.array_equal(data.intensity, np.full((2, 1, 1, 32, 32), 10.0 / 3))


def test_run_images_one_frame_batch_builds_once_and_pads_the_last_probe_batch(monkeypatch):
    from pyslice_amd import Imaging
    pp = [(1.0, 1.5), (2.0, 0.5), (0.5, 0.5)]
    data, created, lines = _run(monkeypatch, Imaging(defocus_series=(0.0, 10.0)), 2, pp, frame_batch=2, probe_batch=2)
    assert (created["n_probes"], created["n_frames"], created["frame_batch"]) == (2, 2, 2)
    assert lines == ["set_kirkland(f8(103,3,4))", "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "build_potentials(f8(2,2,3), i4(2,), 2)",
                     "set_probes(0, xy[0,1])", "propagate_frames(0, 2)", "image_reset(4)",
                     "image_add(0, 2, polar=f8(14,2), aperture_k=0, weight=1, first=0, stride=2, B=2)",
                     "image_add(0, 2, polar=f8(14,2), aperture_k=0, weight=1, first=1, stride=2, B=2)", "image_download(0, 4)",
                     "set_probes(0, xy[2,2])", "propagate_frames(0, 2)", "image_reset(2)",
                     "image_add(0, 2, polar=f8(14,2), aperture_k=0, weight=1, first=0, stride=2, B=1)",
                     "image_add(0, 2, polar=f8(14,2), aperture_k=0, weight=1, first=1, stride=2, B=1)", "image_download(0, 2)"]
    assert data.intensity.shape == (3, 1, 2, 32, 32)


def test_fit_probe_batch_counts_the_image_accumulator(monkeypatch):
    """8 * nx * ny * L * F bytes per probe join the estimate: with room for 7 probes of an F = 1 run, an F = 64 series gets fewer"""
    from pyslice_amd import Imaging, _native, calculators
    monkeypatch.setattr(_native, "Engine", ImagingEngine)
    got = {}
    for F in (1, 64):
        monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: 1.11416e9)
        calc = calculators.MultisliceCalculator(progress=False, imaging=Imaging(defocus_series=tuple(range(F))))
        calc.setup(_trajectory(8), aperture=0.0, voltage_eV=100e3, probe_positions=[(0.3 * i, 0.2 * i) for i in range(7)])
        got[F] = calc._engine.n_probes
        nx = ny = 32
        pitch, batch, nz = 1024, 8, 3
        tables = min(6e9, batch * 2 * (nx // 2 + ny // 2 + 2) * 8.0)

        def need(Pc):
            return Pc * batch * (32.0 * nx * ny + 8.0 * pitch) + Pc * 8.0 * nx * ny * F + batch * 16.0 * nz * nx * ny + tables + 1e9
        Pc = 7
        while Pc > 1 and need(Pc) > 0.9 * 1.11416e9:
            Pc = max(1, Pc // 2)
        assert got[F] == Pc, F
    assert got[64] < got[1]
