"""STEM detectors (MultisliceCalculator(detectors=...)): argument checks, memberships and scan images on the host."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def traj():
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(64, 6, 2, density=0.05, seed=4)


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


@pytest.mark.parametrize("kw", [dict(inner=-1.0), dict(outer=-2.0), dict(inner=40.0, outer=40.0), dict(inner=40.0, outer=30.0),
                                dict(signal="phase"), dict(azimuth=(10.0, 10.0)), dict(azimuth=(0.0, 400.0)), dict(azimuth=(5.0,))])
def test_detector_validation_errors(kw):
    from pyslice_amd import Detector
    with pytest.raises(ValueError):
        Detector("d", **kw)


def test_detector_list_errors():
    from pyslice_amd import Detector
    with pytest.raises(ValueError, match="duplicate"):
        _calc(detectors=[Detector("a"), Detector("a", inner=10.0)])
    with pytest.raises(ValueError, match="at most 16"):
        _calc(detectors=[Detector(f"d{i}") for i in range(17)])
    with pytest.raises(ValueError):
        _calc(detectors=[])
    with pytest.raises(ValueError):
        _calc(detectors=["adf"])
    assert len(_calc(detectors=[Detector(f"d{i}") for i in range(16)])._detectors) == 16


def test_constructor_refusals():
    from pyslice_amd import Detector
    dets = [Detector("bf", outer=10.0)]
    with pytest.raises(ValueError, match="detectors"):
        _calc(probe_batch=8)
    with pytest.raises(ValueError, match="probe_batch"):
        _calc(detectors=dets, probe_batch=0)
    for kw in (dict(cache=True), dict(layers=[1]), dict(stream_tile=4), dict(k_bin=(2, 2))):
        with pytest.raises(ValueError, match="detectors"):
            _calc(detectors=dets, **kw)
    _calc(detectors=dets, k_window=(16, 16), probe_batch=3)          # k_window is allowed


def test_run_names_run_detectors():
    from pyslice_amd import Detector
    with pytest.raises(RuntimeError, match="run_detectors"):
        _calc(detectors=[Detector("bf", outer=10.0)]).run()


def test_several_ranks_refused_before_device_work(traj, monkeypatch):
    from pyslice_amd import Detector, _native, distributed
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))

    def no_engine(*a, **k):
        raise AssertionError("device work before the rank check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = _calc(detectors=[Detector("bf", outer=10.0)])
    with pytest.raises(NotImplementedError, match="ranks"):
        calc.setup(traj, aperture=30.0, voltage_eV=100e3)
    assert calc._engine is None


def test_empty_detector_refused_in_setup(traj, monkeypatch):
    from pyslice_amd import Detector, _native

    def no_engine(*a, **k):
        raise AssertionError("device work before the detector check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = _calc(detectors=[Detector("bf", outer=10.0), Detector("far", inner=5000.0)])
    with pytest.raises(ValueError, match="far"):
        calc.setup(traj, aperture=30.0, voltage_eV=100e3)
    calc = _calc(detectors=[Detector("bf", outer=10.0), Detector("out", inner=60.0)], k_window=(4, 4))
    with pytest.raises(ValueError, match="out"):                      # 60 mrad lies outside a 4 x 4 window
        calc.setup(traj, aperture=30.0, voltage_eV=100e3)


def test_adf_membership_equals_haadf_mask(golden):
    from pyslice_amd import Detector
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.stem_data import detector_bitmask
    g = golden("g9_haadf_32")
    lam = wavelength(float(g["eV"]))
    ca = float(g["collection_angle"])
    det = Detector("adf", inner=ca, signal="amplitude")
    kxs, kys = g["kxs"], g["kys"]
    kx, ky = kxs.astype(np.float64), kys.astype(np.float64)
    want = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2) > (ca * 1e-3) / lam          # haadf_data.py:46-49
    assert np.array_equal(det.member(kxs, kys, lam), want)
    assert np.array_equal(detector_bitmask([Detector("bf", outer=5.0), det], kxs, kys, lam) >> 1, want.astype(np.uint16))
    assert 0 < want.sum() < want.size


def test_azimuthal_segments_partition_the_annulus():
    from pyslice_amd import Detector
    from pyslice_amd.stem_data import detector_bitmask
    k = np.fft.fftshift(np.fft.fftfreq(48, 0.1)).astype(np.float32)
    lam = 0.037
    ring = Detector("ring", inner=5.0, outer=60.0).member(k, k, lam)
    segs = [Detector(f"s{i}", inner=5.0, outer=60.0, azimuth=(90.0 * i, 90.0 * (i + 1))) for i in range(4)]
    bits = detector_bitmask(segs, k, k, lam)
    count = sum(((bits >> i) & 1).astype(int) for i in range(4))
    assert np.array_equal(count, ring.astype(int))
    assert ring.sum() > 100
    # a wrapping segment (315 -> 45 degrees) is the union of the two pieces
    wrap = Detector("w", inner=5.0, outer=60.0, azimuth=(315.0, 45.0)).member(k, k, lam)
    a = Detector("a", inner=5.0, outer=60.0, azimuth=(315.0, 360.0)).member(k, k, lam)
    b = Detector("b", inner=5.0, outer=60.0, azimuth=(0.0, 45.0)).member(k, k, lam)
    assert np.array_equal(wrap, a | b) and not (a & b).any()


def test_inner_zero_includes_the_dc_pixel():
    from pyslice_amd import Detector
    k = np.fft.fftshift(np.fft.fftfreq(33, 0.1)).astype(np.float32)
    assert k[16] == 0
    m = Detector("bf", inner=0.0, outer=10.0).member(k, k, 0.037)
    assert m[16, 16]
    assert not Detector("adf", inner=1.0).member(k, k, 0.037)[16, 16]


def test_detector_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name in ("msl_set_detectors", "msl_detect"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr)
    for sig, v in _native.DET_SIGNALS.items():
        assert re.search(r"#define\s+MSL_DET_" + sig.upper() + r"\s+" + str(v) + r"\b", hdr), sig


def test_stem_image_matches_haadf_nearest_probe_loop():
    from pyslice_amd import Detector, STEMData
    rng = np.random.default_rng(3)
    xs0, ys0 = np.linspace(1.0, 5.0, 4), np.linspace(0.5, 4.0, 5)
    pp = np.array([(x, y) for x in xs0 for y in ys0])[rng.permutation(20)]
    sig = rng.random((20, 3, 2))
    st = STEMData(signals=sig, detectors=[Detector("a"), Detector("b", inner=10.0)], probe_positions=pp,
                  time=np.arange(3) * 0.005, kxs=None, kys=None, probe=None)
    assert np.array_equal(st.xs, xs0) and np.array_equal(st.ys, ys0)
    # HAADFData.calculateADF's assignment (haadf_data.py:81-86) on the frame mean
    per = sig[:, :, 1].mean(axis=1)
    want = np.zeros((4, 5))
    for i, x in enumerate(st.xs):
        for j, y in enumerate(st.ys):
            p = int(np.argmin(np.sqrt(((pp - np.array([x, y])[None, :]) ** 2).sum(axis=1))))
            want[i, j] = per[p]
    assert np.array_equal(st.image("b"), want)
    assert np.array_equal(st.image("a", frames=1), np.array([[sig[np.argmin(((pp - (x, y)) ** 2).sum(1)), 1, 0] for y in st.ys] for x in st.xs]))
    with pytest.raises(KeyError):
        st.image("c")
