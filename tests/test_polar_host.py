"""Polar detector (MultisliceCalculator(polar=...)) on the host: the request, the bin map against Detector.member, the reference
sums, msl_polar_layout (no device), the ABI, the calculator's refusals and call sequence, and PolarData."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.037
NONE = 0xFFFF


def _axes(shape):
    kx = np.fft.fftshift(np.fft.fftfreq(shape[0], 0.1)).astype(np.float32)
    ky = np.fft.fftshift(np.fft.fftfreq(shape[1], 0.1)).astype(np.float32)
    return kx, ky


def _theta(kx, ky):
    """scattering angle of every pixel in mrad, from q as Detector.member forms it"""
    q = np.sqrt(kx.astype(np.float64)[:, None] ** 2 + ky.astype(np.float64)[None, :] ** 2)
    return q, q * LAM / 1e-3


# ------------------------------------------------------------------ 1. the request
@pytest.mark.parametrize("kw", [dict(outer=-1.0), dict(outer=float("nan")), dict(outer=float("inf")), dict(outer=10.0, inner=-1.0),
                                dict(outer=10.0, inner=float("nan")), dict(outer=10.0, inner=10.0), dict(outer=10.0, inner=12.0),
                                dict(outer=10.0, step=0.0), dict(outer=10.0, step=-1.0), dict(outer=10.0, step=float("inf")),
                                dict(outer=10.0, n_azimuthal=0), dict(outer=10.0, n_azimuthal=-3), dict(outer=10.0, n_azimuthal=2.5),
                                dict(outer=10.0, rotation=float("nan")), dict(outer=4097.0), dict(outer=1025.0, n_azimuthal=4),
                                dict(outer="10")])
def test_polar_detector_refusals(kw):
    from pyslice_amd import PolarDetector
    with pytest.raises(ValueError):
        PolarDetector(**kw)


def test_polar_detector_rings_edges_bins():
    from pyslice_amd import PolarDetector
    p = PolarDetector(outer=40, step=1)
    assert (p.n_rings, p.n_bins) == (40, 40) and np.array_equal(p.edges, np.arange(41.0))
    p = PolarDetector(inner=10, outer=25.5, step=2)
    assert p.n_rings == 8 and np.array_equal(p.edges, 10.0 + 2.0 * np.arange(9)) and p.edges[-1] == 26.0      # not `outer`
    p = PolarDetector(outer=60, step=2, n_azimuthal=4, per_frame=True)
    assert (p.n_rings, p.n_azimuthal, p.n_bins, p.per_frame) == (30, 4, 120, True)
    assert PolarDetector(outer=4096.0).n_bins == 4096 and PolarDetector(outer=1024.0, n_azimuthal=4).n_bins == 4096
    assert PolarDetector(outer=1.1, step=0.1).n_rings == 11          # (1.1 / 0.1 = 11.000000000000002)
    assert PolarDetector(outer=0.35, step=0.1).n_rings == 4
    with pytest.raises(Exception):
        p.outer = 3.0                                                # frozen
    assert PolarDetector(outer=10.0) == PolarDetector(outer=10, step=1.0, inner=0, n_azimuthal=1, rotation=0.0, per_frame=False)


# ------------------------------------------------------------------ 2. the bin map
@pytest.mark.parametrize("shape", [(45, 63), (32, 32)])
@pytest.mark.parametrize("kw", [dict(outer=40.0, step=1.0), dict(inner=10.0, outer=25.5, step=2.0, n_azimuthal=3),
                                dict(outer=30.0, step=5.0, n_azimuthal=12, rotation=15.0), dict(outer=400.0, step=50.0, n_azimuthal=4)])
def test_bins_partition_the_annulus(shape, kw):
    from pyslice_amd import PolarDetector, polar_bins
    from pyslice_amd.polar_data import bin_counts
    pol = PolarDetector(**kw)
    kx, ky = _axes(shape)
    bins = polar_bins(pol, kx, ky, LAM)
    assert bins.shape == shape and bins.dtype == np.uint16
    q, _ = _theta(kx, ky)
    e = (pol.edges * 1e-3) / LAM
    inside = (q > e[0]) & (q <= e[-1])
    if pol.inner == 0:
        inside |= q == 0
    assert np.array_equal(bins != NONE, inside)                      # in exactly one bin, or in none
    assert bins[inside].max() < pol.n_bins
    counts = bin_counts(bins, pol.n_bins)
    assert counts.shape == (pol.n_bins,) and counts.dtype == np.int64 and counts.sum() == inside.sum()
    # the ring and the sector of every pixel inside, by their definitions
    ring = bins[inside].astype(int) // pol.n_azimuthal
    assert ((q[inside] > e[ring]) | ((q[inside] == 0) & (ring == 0))).all() and (q[inside] <= e[ring + 1]).all()
    dc = (shape[0] // 2, shape[1] // 2)
    assert q[dc] == 0
    assert (bins[dc] // pol.n_azimuthal == 0) if pol.inner == 0 else (bins[dc] == NONE)


@pytest.mark.parametrize("shape", [(45, 63), (32, 32)])
def test_bins_are_detector_members(shape):
    """the union of the bins between two edges is exactly Detector.member of the detector with those edges"""
    from pyslice_amd import Detector, PolarDetector, polar_bins, polar_signals
    kx, ky = _axes(shape)
    rng = np.random.default_rng(5)
    W = (rng.standard_normal((2, 3) + shape) + 1j * rng.standard_normal((2, 3) + shape)).astype(np.complex64)
    I = np.abs(W.astype(np.complex128)) ** 2

    def check(pol, det, rings, sectors):
        bins = polar_bins(pol, kx, ky, LAM)
        A = pol.n_azimuthal
        ids = [r * A + a for r in rings for a in sectors]
        m = det.member(kx, ky, LAM)
        assert m.any(), det
        assert np.array_equal(np.isin(bins, ids), m), (pol, det)
        got = polar_signals(W, bins, pol.n_bins)[..., ids].sum(axis=-1)
        want = (I * m.astype(np.float64)).sum(axis=(-2, -1))
        assert np.allclose(got, want, rtol=1e-13, atol=0)

    pol = PolarDetector(outer=240.0, step=20.0)
    check(pol, Detector("bf", outer=100.0), range(0, 5), [0])
    check(pol, Detector("adf", inner=100.0, outer=240.0), range(5, 12), [0])
    check(pol, Detector("ring", inner=40.0, outer=60.0), [2], [0])
    pol = PolarDetector(inner=10.0, outer=25.5, step=2.0)
    check(pol, Detector("abf", inner=12.0, outer=26.0), range(1, 8), [0])
    pol = PolarDetector(outer=120.0, step=20.0, n_azimuthal=4)
    for a, az in enumerate([(0, 90), (90, 180), (180, 270), (270, 360)]):
        check(pol, Detector(f"q{a}", outer=120.0, azimuth=az), range(6), [a])
        check(pol, Detector(f"r{a}", inner=40.0, outer=80.0, azimuth=az), [2, 3], [a])
    pol = PolarDetector(outer=120.0, step=20.0, n_azimuthal=8, rotation=45.0)
    check(pol, Detector("seg", outer=120.0, azimuth=(45, 135)), range(6), [0, 1])
    check(pol, Detector("wrap", inner=20.0, outer=120.0, azimuth=(315, 45)), range(1, 6), [6, 7])


def test_polar_signals_shapes_and_empty_bins():
    from pyslice_amd import polar_signals
    rng = np.random.default_rng(6)
    W = (rng.standard_normal((4, 3, 5)) + 1j * rng.standard_normal((4, 3, 5))).astype(np.complex64)
    bins = np.full((3, 5), NONE, dtype=np.uint16)
    bins[0, 1], bins[2, 4], bins[1, 1] = 6, 2, 6
    got = polar_signals(W, bins, 9)
    assert got.shape == (4, 9) and got.dtype == np.float64
    I = np.abs(W.astype(np.complex128)) ** 2
    assert np.array_equal(got[:, 6], I[:, 0, 1] + I[:, 1, 1]) and np.array_equal(got[:, 2], I[:, 2, 4])
    assert not got[:, [0, 1, 3, 4, 5, 7, 8]].any()
    assert not polar_signals(W, np.full((3, 5), NONE, dtype=np.uint16), 4).any()
    with pytest.raises(ValueError):
        polar_signals(W, bins, 6)
    with pytest.raises(ValueError):
        polar_signals(W, bins[:2], 9)


# ------------------------------------------------------------------ 3. msl_polar_layout: host only
@pytest.fixture(scope="module")
def lib():
    from pyslice_amd import build_native, _native
    build_native.build()
    return _native.load()


def _layout_maps():
    rng = np.random.default_rng(7)
    maps = []
    for n_bins in (1, 7, 4096):
        m = rng.integers(0, n_bins, size=5000).astype(np.uint16)
        m[rng.random(5000) < 0.3] = NONE
        maps.append((f"random{n_bins}", m, n_bins))
    maps.append(("all_none", np.full(300, NONE, dtype=np.uint16), 5))
    m = rng.choice([2, 5, 11], size=777).astype(np.uint16)
    maps.append(("empty_bins", m, 13))
    maps.append(("one_pixel", np.array([3], dtype=np.uint16), 4))
    maps.append(("one_pixel_none", np.array([NONE], dtype=np.uint16), 4))
    return maps


@pytest.mark.parametrize("name,m,n_bins", _layout_maps(), ids=[c[0] for c in _layout_maps()])
def test_layout_is_the_stable_sort(lib, name, m, n_bins):
    from pyslice_amd import _native
    order, seg = _native.polar_layout(m, n_bins)
    keep = np.flatnonzero(m != NONE)
    want = keep[np.argsort(m[keep], kind="stable")]
    assert order.dtype == np.uint32 and seg.dtype == np.int64 and seg.shape == (n_bins + 1,)
    assert np.array_equal(order, want)
    assert np.array_equal(seg, np.r_[0, np.cumsum(np.bincount(m[keep], minlength=n_bins))])
    assert seg[-1] == keep.size
    for b in (0, n_bins // 2, n_bins - 1):
        assert np.array_equal(order[seg[b]:seg[b + 1]], np.flatnonzero(m == b))


def test_layout_refusals(lib):
    from pyslice_amd import _native
    m = np.array([0, 1, 4, 2], dtype=np.uint16)
    with pytest.raises(ValueError, match="bin id"):
        _native.polar_layout(m, 4)                                   # a bin id equal to n_bins
    order, seg = np.zeros(4, np.uint32), np.zeros(5, np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    assert lib.msl_polar_layout(ptr(m), 4, 4, ptr(order), ptr(seg)) == _native.MSL_ERR_INVALID
    seg6 = np.zeros(6, np.int64)
    assert lib.msl_polar_layout(ptr(m), 4, 5, ptr(order), ptr(seg6)) == _native.MSL_OK and seg6[-1] == 4
    for n_bins in (0, -1, 4097):
        assert lib.msl_polar_layout(ptr(m), 4, n_bins, ptr(order), ptr(seg)) == _native.MSL_ERR_INVALID
    assert lib.msl_polar_layout(None, 4, 5, ptr(order), ptr(seg)) == _native.MSL_ERR_INVALID
    assert lib.msl_polar_layout(ptr(m), -1, 5, ptr(order), ptr(seg)) == _native.MSL_ERR_INVALID
    assert lib.msl_polar_layout(ptr(m), 4, 5, None, ptr(seg)) == _native.MSL_ERR_INVALID


# ------------------------------------------------------------------ 4. the ABI
def test_polar_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name in ("msl_polar_layout", "msl_set_polar", "msl_polar_detect"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr) and _native.ABI_VERSION == 3
    assert re.search(r"#define\s+MSL_POLAR_NONE\s+0xFFFF\b", hdr) and _native.POLAR_NONE == 0xFFFF
    assert re.search(r"#define\s+MSL_POLAR_MAX_BINS\s+4096\b", hdr) and _native.POLAR_MAX_BINS == 4096
    assert callable(getattr(_native.Engine, "set_polar")) and callable(getattr(_native.Engine, "polar_detect"))


# ------------------------------------------------------------------ 5. the calculator
PP = [(0.3 * i, 0.2 * i) for i in range(5)]


class PolarEngine(RecordingEngine):
    """answers polar_detect with 1 + frame slot + bin / 1000 for every probe"""

    def __getattr__(self, name):
        call = RecordingEngine.__getattr__(self, name)
        if name == "set_polar":
            def set_polar(bins, n_bins):
                self._n_bins = n_bins
                return call(bins, n_bins)
            return set_polar
        if name == "polar_detect":
            def polar_detect(t0, count, B=None):
                call(t0, count, B=B)
                return np.ones((B, count, self._n_bins)) + np.arange(count)[None, :, None] + np.arange(self._n_bins)[None, None, :] / 1000.0
            return polar_detect
        return call


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", PolarEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)


def test_constructor_refusals_and_allowances():
    from pyslice_amd import Aberrations, Detector, Diffraction, Imaging, PolarDetector, Spectroscopy
    from pyslice_amd.prism import Prism
    pol = PolarDetector(outer=40.0)
    for kw in (dict(cache=True), dict(layers=[1]), dict(stream_tile=4), dict(k_bin=(2, 2)), dict(diffraction=Diffraction()),
               dict(imaging=Imaging()), dict(spectroscopy=Spectroscopy([Detector("bf", outer=10.0)]))):
        with pytest.raises(ValueError, match="polar"):
            _calc(polar=pol, **kw)
    with pytest.raises(ValueError, match="PolarDetector"):
        _calc(polar=(40.0, 1.0))
    with pytest.raises(ValueError, match="detectors"):
        _calc(probe_batch=8)                                         # no probe-batch mode: still refused, in the same words
    with pytest.raises(ValueError, match="probe_batch"):
        _calc(polar=pol, probe_batch=0)
    _calc(polar=pol, probe_batch=3)                                  # probe_batch with polar alone
    _calc(polar=pol, k_window=(16, 16), aberrations=Aberrations(defocus=50.0), frame_batch=2, probe_batch=3, prism=Prism(1),
          detectors=[Detector("bf", outer=10.0)])


def test_run_methods_name_run_polar():
    from pyslice_amd import Detector, PolarDetector
    pol = PolarDetector(outer=40.0)
    with pytest.raises(RuntimeError, match="run_polar"):
        _calc(polar=pol).run()
    with pytest.raises(RuntimeError, match="polar="):
        _calc().run_polar()
    with pytest.raises(RuntimeError, match="setup"):
        _calc(polar=pol).run_polar()
    with pytest.raises(RuntimeError, match="diffraction="):
        _calc(polar=pol).run_diffraction()                           # the other modes keep their own errors
    with pytest.raises(RuntimeError, match="run_detectors"):
        _calc(polar=pol, detectors=[Detector("bf", outer=10.0)]).run()


def test_run_detectors_without_detectors_names_run_polar(recorder):
    from pyslice_amd import PolarDetector
    calc = _calc(polar=PolarDetector(outer=40.0))
    calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    with pytest.raises(RuntimeError, match="run_polar"):
        calc.run_detectors()


def test_setup_refusals_before_device_work(monkeypatch):
    from pyslice_amd import PolarDetector, _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("device work before the check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = _calc(polar=PolarDetector(inner=500.0, outer=600.0, step=10.0))       # the 32 x 32 spectrum ends near 260 mrad
    with pytest.raises(ValueError, match="no stored pixel"):
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    assert calc._engine is None
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    calc = _calc(polar=PolarDetector(outer=40.0))
    with pytest.raises(NotImplementedError, match="polar.*ranks"):
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    assert calc._engine is None


@pytest.mark.parametrize("per_frame", [False, True])
def test_call_sequence_and_frame_mean(recorder, per_frame):
    """5 probes x 3 frames at probe_batch=2, frame_batch=2: one set_polar, one polar_detect(0, n, B=real) per probe batch and frame
    batch; the mean over the frames, or every frame"""
    from pyslice_amd import PolarData, PolarDetector
    pol = PolarDetector(outer=60.0, step=20.0, n_azimuthal=2, per_frame=per_frame)
    calc = _calc(polar=pol, probe_batch=2, frame_batch=2)
    calc.setup(_trajectory(3), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    assert calc.probe_batch == 2
    res = calc.run_polar()
    lines = format_calls(calc._engine.calls, PP)
    assert [l for l in lines if l.startswith("set_polar")] == ["set_polar(u2(1024,), 6)"]
    assert lines.index("set_polar(u2(1024,), 6)") > max(i for i, l in enumerate(lines) if l.startswith(("set_kirkland", "set_slices", "set_aberrations")))
    assert not [l for l in lines if l.startswith(("detect", "set_detectors", "diffract"))]
    keep = [l for l in lines if l.startswith(("build_potential", "set_probes", "propagate_frame", "polar_detect"))]
    want = []
    for s0, n in ((0, 2), (2, 1)):
        want.append("build_potentials(f8(2,%d,3), i4(%d,), 2)" % ((calc.trajectory.n_atoms,) * 2) if n == 2 else
                    "build_potentials(f8(1,%d,3), i4(%d,), 2)" % ((calc.trajectory.n_atoms,) * 2))
        for xy, real in (("xy[0,1]", 2), ("xy[2,3]", 2), ("xy[4,4]", 1)):
            want += [f"set_probes(30, {xy})", f"propagate_frames(0, {n})", f"polar_detect(0, {n}, B={real})"]
    assert keep == want
    assert isinstance(res, PolarData) and res.stem is None and res.polar is pol
    bins = np.arange(6).reshape(3, 2) / 1000.0
    if per_frame:
        assert res.signals.shape == (5, 3, 3, 2)
        for t, slot in enumerate((0, 1, 0)):
            assert np.array_equal(res.signals[:, t], np.broadcast_to(1.0 + slot + bins, (5, 3, 2)))
    else:
        assert res.signals.shape == (5, 3, 2)
        assert np.allclose(res.signals, np.broadcast_to(4.0 / 3.0 + bins, (5, 3, 2)), rtol=1e-15, atol=0)
    assert res.counts.shape == (3, 2) and res.counts.dtype == np.int64 and res.counts.sum() > 0
    assert np.array_equal(res.edges, [0.0, 20.0, 40.0, 60.0]) and len(res.time) == 3


def test_stem_is_present_exactly_with_detectors(recorder):
    from pyslice_amd import Detector, PolarDetector, STEMData
    dets = [Detector("bf", outer=20.0), Detector("adf", inner=40.0)]
    calc = _calc(polar=PolarDetector(outer=60.0, step=20.0), detectors=dets, probe_batch=2, frame_batch=2)
    calc.setup(_trajectory(3), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    res = calc.run_polar()
    assert isinstance(res.stem, STEMData) and res.stem.signals.shape == (5, 3, 2) and res.stem.detectors == dets
    lines = format_calls(calc._engine.calls, PP)
    assert len([l for l in lines if l.startswith("set_detectors")]) == 1 and len([l for l in lines if l.startswith("set_polar")]) == 1
    pairs = [l for l in lines if l.startswith(("polar_detect", "detect"))]
    assert pairs[:4] == ["polar_detect(0, 2, B=2)", "detect(0, 2, B=2)", "polar_detect(0, 2, B=2)", "detect(0, 2, B=2)"] and len(pairs) == 12


def test_prism_takes_the_prism_loop(recorder):
    from pyslice_amd import PolarDetector
    from pyslice_amd.prism import Prism
    calc = _calc(polar=PolarDetector(outer=60.0, step=20.0), probe_batch=2, prism=Prism(1))
    calc.setup(_trajectory(2), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    res = calc.run_polar()
    lines = format_calls(calc._engine.calls, PP)
    assert len([l for l in lines if l.startswith("smatrix_build")]) == 2
    assert [l for l in lines if l.startswith("polar_detect")] == ["polar_detect(0, 1, B=2)", "polar_detect(0, 1, B=2)", "polar_detect(0, 1, B=1)"] * 2
    assert res.signals.shape == (5, 3, 1)


def test_output_scratch_is_counted_in_the_probe_batch(monkeypatch):
    """8 * Pc * batch * n_bins bytes: a free-memory figure between the need without and with it halves the probe batch"""
    from pyslice_amd import PolarDetector, _native, calculators
    monkeypatch.setattr(_native, "Engine", PolarEngine)
    pp = [(0.01 * i, 0.0) for i in range(256)]

    def probe_batch(polar, free_b):
        monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: free_b)
        calc = _calc(polar=polar, frame_batch=1)
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        return calc._engine.n_probes
    small, large = PolarDetector(outer=40.0, step=40.0), PolarDetector(outer=4096.0, step=1.0)
    calc = _calc(polar=small, frame_batch=1)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    fixed = calc._phase_table_bytes(1) + 16.0 * 3 * 32 * 32 + 1e9
    per_probe = 32.0 * 32 * 32 + 8.0 * 1024
    free_b = (fixed + 256 * (per_probe + 8.0 * 2048)) / 0.9          # room for 2048 bins per image, not for 4096
    assert probe_batch(small, free_b) == 256
    assert probe_batch(large, free_b) == 128


# ------------------------------------------------------------------ 6. PolarData on a hand-made array
def _data(per_frame, A=4, rotation=0.0):
    from pyslice_amd import PolarData, PolarDetector
    pol = PolarDetector(inner=4.0, outer=20.0, step=4.0, n_azimuthal=A, rotation=rotation, per_frame=per_frame)
    rng = np.random.default_rng(8)
    P, T, R = 6, 3, 4
    sig = rng.random((P, T, R, A) if per_frame else (P, R, A))
    pp = [(float(x), float(y)) for x in (1.0, 2.0, 3.0) for y in (0.5, 1.5)]
    kx, ky = _axes((32, 32))
    return PolarData(signals=sig, polar=pol, counts=np.ones((R, A), dtype=np.int64), edges=pol.edges, probe_positions=pp,
                     time=np.arange(T) * 0.005, kxs=kx, kys=ky, probe=None)


def _close(a, b):
    """equal but for the order of a float64 sum"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.allclose(a, b, rtol=1e-14, atol=0)


def test_integrate_profile_image():
    pd = _data(per_frame=False)
    s = pd.signals
    assert _close(pd.edges, [4.0, 8.0, 12.0, 16.0, 20.0])
    assert _close(pd.integrate(4.0), s.sum(axis=(1, 2)))
    assert _close(pd.integrate(8.0, 16.0), s[:, 1:3].sum(axis=(1, 2)))
    assert _close(pd.integrate(8.0 + 5e-10, 16.0 - 5e-10), s[:, 1:3].sum(axis=(1, 2)))
    assert _close(pd.integrate(4.0, 8.0, azimuth=(90, 270)), s[:, 0:1, 1:3].sum(axis=(1, 2)))
    assert _close(pd.integrate(4.0, azimuth=(270, 90)), s[:, :, [3, 0]].sum(axis=(1, 2)))
    assert _close(pd.integrate(4.0, azimuth=(0, 360)), s.sum(axis=(1, 2)))
    assert _close(pd.profile(), s.sum(axis=-1).mean(axis=0)) and pd.profile().shape == (4,)
    assert _close(pd.profile(2), s[2].sum(axis=-1))
    assert _close(pd.xs, [1.0, 2.0, 3.0]) and _close(pd.ys, [0.5, 1.5])
    assert _close(pd.image(8.0, 12.0), s[:, 1].sum(axis=-1).reshape(3, 2))
    with pytest.raises(ValueError, match="per_frame"):
        pd.image(8.0, 12.0, frames=[0])
    with pytest.raises(ValueError, match="per_frame"):
        pd.to_stem([])


def test_integrate_refuses_what_is_not_an_edge():
    pd = _data(per_frame=False)
    with pytest.raises(ValueError, match=r"inner=9.0.*8 and 12 mrad"):
        pd.integrate(9.0)
    with pytest.raises(ValueError, match=r"outer=18.5.*16 and 20 mrad"):
        pd.integrate(8.0, 18.5)
    with pytest.raises(ValueError, match=r"inner=0.0.*4 and 8 mrad"):
        pd.integrate(0.0)                                             # below the first edge
    with pytest.raises(ValueError, match=r"outer=25.0.*16 and 20 mrad"):
        pd.integrate(8.0, 25.0)
    with pytest.raises(ValueError, match="exceed"):
        pd.integrate(12.0, 8.0)
    with pytest.raises(ValueError, match=r"45.0 degrees is not a sector boundary.*0 and 90"):
        pd.integrate(4.0, azimuth=(45, 90))
    with pytest.raises(ValueError):
        pd.integrate(4.0, azimuth=(90, 90))
    rot = _data(per_frame=False, A=8, rotation=45.0)
    assert _close(rot.integrate(4.0, azimuth=(45, 135)), rot.signals[:, :, 0:2].sum(axis=(1, 2)))
    assert _close(rot.integrate(4.0, azimuth=(315, 45)), rot.signals[:, :, 6:8].sum(axis=(1, 2)))
    with pytest.raises(ValueError, match="sector boundary"):
        rot.integrate(4.0, azimuth=(30, 135))


def test_per_frame_image_and_to_stem():
    from pyslice_amd import Detector, STEMData
    pd = _data(per_frame=True)
    s = pd.signals
    assert pd.integrate(8.0, 16.0).shape == (6, 3)
    assert _close(pd.profile(), s.sum(axis=-1).mean(axis=1).mean(axis=0))
    assert np.allclose(pd.image(8.0, 12.0), s[:, :, 1].sum(axis=-1).mean(axis=1).reshape(3, 2), rtol=1e-15)
    assert np.allclose(pd.image(8.0, 12.0, frames=[0, 2]), s[:, [0, 2], 1].sum(axis=-1).mean(axis=1).reshape(3, 2), rtol=1e-15)
    assert _close(pd.image(8.0, 12.0, frames=1), s[:, 1, 1].sum(axis=-1).reshape(3, 2))
    dets = [Detector("ring", inner=4.0, outer=12.0), Detector("q1", inner=8.0, outer=20.0, azimuth=(90, 180))]
    st = pd.to_stem(dets)
    assert isinstance(st, STEMData) and st.signals.shape == (6, 3, 2) and st.detectors == dets
    assert _close(st.signals[..., 0], s[:, :, 0:2].sum(axis=(2, 3)))
    assert _close(st.signals[..., 1], s[:, :, 1:4, 1].sum(axis=2))
    assert np.allclose(st.image("ring"), pd.image(4.0, 12.0), rtol=1e-15)
    with pytest.raises(ValueError, match="signal"):
        pd.to_stem([Detector("a", inner=4.0, outer=8.0, signal="amplitude")])
    with pytest.raises(ValueError, match="outer"):
        pd.to_stem([Detector("a", inner=4.0)])
    with pytest.raises(ValueError, match="ring edge"):
        pd.to_stem([Detector("a", inner=5.0, outer=8.0)])


def test_polar_data_checks_its_shape():
    from pyslice_amd import PolarData, PolarDetector
    pol = PolarDetector(outer=8.0, step=4.0)
    with pytest.raises(ValueError, match="rings"):
        PolarData(signals=np.zeros((3, 2, 2)), polar=pol, counts=np.zeros((2, 1), np.int64), edges=pol.edges, probe_positions=[(0.0, 0.0)] * 3,
                  time=np.zeros(1), kxs=None, kys=None, probe=None)
