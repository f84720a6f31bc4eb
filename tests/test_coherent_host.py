"""Elastic / thermal-diffuse split of the diffraction patterns (Diffraction(split=True)): the ABI entries, the request and
DiffractionData with an elastic part, on the host."""
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.037


# ------------------------------------------------------------------ 1. the ABI
def test_coherent_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name in ("msl_coherent_reset", "msl_coherent_add", "msl_coherent_finish"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr)
    assert _native.ABI_VERSION == 3
    for meth in ("coherent_reset", "coherent_add", "coherent_finish"):
        assert callable(getattr(_native.Engine, meth))


# ------------------------------------------------------------------ 2. the request
@pytest.mark.parametrize("bad", [1, 0, "yes", None, (True,), 1.0, np.int64(1)])
def test_split_must_be_a_bool(bad):
    from pyslice_amd import Diffraction
    with pytest.raises(ValueError, match="split"):
        Diffraction(bin=(2, 2), split=bad)


def test_split_request_and_repr():
    from pyslice_amd import Diffraction
    assert Diffraction().split is False
    assert Diffraction(bin=(2, 3), split=np.bool_(True)).split is True
    assert Diffraction(bin=(4, 5), split=True).bin == (4, 5)
    assert repr(Diffraction(bin=(4, 5))) == "Diffraction(bin=(4, 5))"
    assert repr(Diffraction(bin=(4, 5), split=False)) == "Diffraction(bin=(4, 5))"          # unchanged without the split
    assert repr(Diffraction(bin=(4, 5), split=True)) == "Diffraction(bin=(4, 5), split=True)"
    with pytest.raises(ValueError, match="bin"):
        Diffraction(bin=(0, 1), split=True)


def test_split_keeps_the_refusals_of_a_diffraction_run():
    from pyslice_amd import Diffraction
    from pyslice_amd.calculators import MultisliceCalculator
    d = Diffraction(bin=(2, 2), split=True)
    for kw in (dict(cache=True), dict(layers=[1]), dict(stream_tile=4), dict(k_bin=(2, 2))):
        with pytest.raises(ValueError, match="diffraction"):
            MultisliceCalculator(progress=False, diffraction=d, **kw)
    with pytest.raises(RuntimeError, match="run_diffraction"):
        MultisliceCalculator(progress=False, diffraction=d).run()
    with pytest.raises(RuntimeError, match="setup"):
        MultisliceCalculator(progress=False, diffraction=d).run_diffraction()


# ------------------------------------------------------------------ 3. DiffractionData with an elastic part
def _data(P=12, shape=(24, 20), bin=(2, 5), seed=5, split=True):
    from pyslice_amd import DiffractionData
    from pyslice_amd.diffraction_data import bin_centres
    rng = np.random.default_rng(seed)
    kx = np.fft.fftshift(np.fft.fftfreq(shape[0], 0.1)).astype(np.float32)
    ky = np.fft.fftshift(np.fft.fftfreq(shape[1], 0.1)).astype(np.float32)
    pp = np.array([(x, y) for x in np.linspace(1.0, 4.0, 3) for y in np.linspace(0.5, 3.5, 4)])[rng.permutation(12)][:P]
    el = rng.random((P, shape[0] // bin[0], shape[1] // bin[1]))
    tot = el + 0.3 * rng.random(el.shape)
    return DiffractionData(intensity=tot, kxs=bin_centres(kx, bin[0]), kys=bin_centres(ky, bin[1]), bin=bin, n_frames=4,
                           probe_positions=pp, probe=None, wavelength=LAM, elastic=el if split else None)


def test_tds_is_the_plain_difference():
    dd = _data()
    assert np.array_equal(dd.tds, dd.intensity - dd.elastic)
    # not clamped: a value below zero stays below zero
    dd.elastic[3, 2, 1] = dd.intensity[3, 2, 1] * (1.0 + 2e-7)
    assert dd.tds[3, 2, 1] < 0.0
    assert np.array_equal(dd.tds, dd.intensity - dd.elastic)


def test_parts():
    dd = _data()
    for name, want in (("total", dd.intensity), ("elastic", dd.elastic), ("tds", dd.intensity - dd.elastic)):
        part = dd.part(name)
        assert type(part) is type(dd)
        assert np.array_equal(part.intensity, want), name
        assert part.elastic is None
        assert part.bin == dd.bin and part.n_frames == dd.n_frames and part.wavelength == dd.wavelength
        assert np.array_equal(part.kxs, dd.kxs) and np.array_equal(part.kys, dd.kys)
        assert np.array_equal(np.asarray(part.probe_positions), np.asarray(dd.probe_positions))
        assert np.array_equal(part.xs, dd.xs) and np.array_equal(part.ys, dd.ys)
        assert np.array_equal(part.pacbed(), want.mean(axis=0)), name
        pp = np.asarray(dd.probe_positions)
        assert np.array_equal(part.pattern(pp[5, 0], pp[5, 1]), want[5])
        with pytest.raises(ValueError, match="split"):
            part.part("elastic")                                  # a part has no parts of its own
    assert np.array_equal(dd.part("elastic").pacbed(), dd.elastic.mean(axis=0))
    for bad in ("TDS", "inelastic", "", None, 0):
        with pytest.raises(ValueError, match="part"):
            dd.part(bad)


def test_parts_need_the_split():
    dd = _data(split=False)
    assert dd.elastic is None
    with pytest.raises(ValueError, match="split"):
        dd.tds
    for name in ("total", "elastic", "tds"):
        with pytest.raises(ValueError, match="split"):
            dd.part(name)
    with pytest.raises(ValueError, match="part"):
        dd.part("nothing")
    assert np.array_equal(dd.pacbed(), dd.intensity.mean(axis=0))              # everything else as before


def test_virtual_detectors_on_each_part_are_direct_sums():
    from pyslice_amd import Detector
    dd = _data()
    det = Detector("adf", inner=20.0, outer=90.0)
    cx, cy = np.asarray(dd.kxs, dtype=np.float64), np.asarray(dd.kys, dtype=np.float64)
    q = np.sqrt(cx[:, None] ** 2 + cy[None, :] ** 2)
    m = (q > 20e-3 / LAM) & (q <= 90e-3 / LAM)
    assert 0 < m.sum() < m.size
    for name, arr in (("total", dd.intensity), ("elastic", dd.elastic), ("tds", dd.intensity - dd.elastic)):
        want = np.array([arr[p][m].sum() for p in range(arr.shape[0])])
        assert np.allclose(dd.part(name).virtual(det), want, rtol=1e-13, atol=0), name
        assert dd.part(name).image(det).shape == (3, 4)
    # the parts add up on every detector
    assert np.allclose(dd.part("elastic").virtual(det) + dd.part("tds").virtual(det), dd.virtual(det), rtol=1e-13, atol=0)


def test_elastic_must_have_the_shape_of_the_intensity():
    from pyslice_amd import DiffractionData
    with pytest.raises(ValueError, match="shape"):
        DiffractionData(intensity=np.zeros((2, 4, 4)), kxs=np.zeros(4, np.float32), kys=np.zeros(4, np.float32), bin=(1, 1), n_frames=1,
                        probe_positions=[(0.0, 0.0), (1.0, 1.0)], probe=None, wavelength=LAM, elastic=np.zeros((2, 4, 2)))


# ------------------------------------------------------------------ 4. the frames-inside loop, on an engine that only records its calls
@pytest.mark.parametrize("n_frames,frame_batch,builds", [(5, 2, 9), (2, 2, 1), (3, 1, 9)])
def test_frames_inside_loop_order(monkeypatch, n_frames, frame_batch, builds):
    """probe batches outside, frame batches inside: one set_probes and one reset per probe batch, an add after every slice loop, one
    finish per probe batch over the real probes; the potentials once per probe batch and frame batch, or once in all when the
    trajectory is a single frame batch"""
    from pyslice_amd import Diffraction, _native
    from pyslice_amd.calculators import MultisliceCalculator
    from pyslice_amd.synthetic import synthetic_trajectory
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    tr = synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)
    pp = [(0.3 * i, 0.2 * i) for i in range(7)]
    calc = MultisliceCalculator(progress=False, diffraction=Diffraction(bin=(4, 8), split=True), probe_batch=3, frame_batch=frame_batch)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    dd = calc.run_diffraction()
    names = [c[0] for c in calc._engine.calls if c[0] not in ("set_kirkland", "set_slices", "set_aberrations")]
    per_probe_batch = -(-n_frames // frame_batch)
    assert names.count("set_probes") == names.count("coherent_reset") == names.count("coherent_finish") == 3
    assert names.count("coherent_add") == names.count("diffract") == 3 * per_probe_batch
    assert names.count("build_potential") + names.count("build_potentials") == builds
    if builds == 1:
        assert names[0].startswith("build_potential")
    first = names.index("set_probes")
    assert names[first + 1] == "coherent_reset"
    for i, n in enumerate(names):
        if n == "coherent_add":
            assert names[i - 1] == "diffract" and names[i - 2].startswith("propagate_frame")
        if n == "coherent_finish":
            assert names[i - 1] == "coherent_add"
    adds = [c for c in calc._engine.calls if c[0] == "coherent_add"]
    assert [c[2]["B"] for c in adds] == [3] * (2 * per_probe_batch) + [1] * per_probe_batch          # the padded last batch: real probes only
    assert sum(c[1][1] for c in adds[:per_probe_batch]) == n_frames                                    # every frame of a probe batch is added
    fins = [c for c in calc._engine.calls if c[0] == "coherent_finish"]
    assert [(c[1][0], c[2]["B"]) for c in fins] == [(n_frames, 3), (n_frames, 3), (n_frames, 1)]
    assert dd.elastic.shape == dd.intensity.shape == (7, 8, 4) and (dd.elastic == 0.25).all() and np.allclose(dd.intensity, 1.0)
    assert np.allclose(dd.tds, 0.75)
