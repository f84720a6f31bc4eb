"""Thickness series of the probe-batch modes (MultisliceCalculator(thickness=...)) on the host: the request, the refusals, the call
order and result shapes of the three run methods on a recording engine, the layered result objects, the ABI, and the device-free
layout of the staging area."""
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = [(0.3 * i, 0.2 * i) for i in range(5)]


# ------------------------------------------------------------------ 1. the request
def test_thickness_resolves_sorted_unique_with_the_exit_last():
    from pyslice_amd.thickness import Thickness, as_thickness
    assert Thickness(slices=[3, 1, 3, 0]).resolve(6) == [0, 1, 3, 5]
    assert Thickness(slices=[5, 2]).resolve(6) == [2, 5]                 # the exit is not listed twice
    assert Thickness(slices=[]).resolve(6) == [5]
    assert as_thickness([4, np.int64(2)]).resolve(6) == [2, 4, 5]
    assert as_thickness((1,)).patterns == "position"
    t = Thickness(every=2, patterns="pacbed")
    assert as_thickness(t) is t and t.resolve(6) == [1, 3, 5] and t.resolve(5) == [1, 3, 4]
    assert Thickness(every=1).resolve(3) == [0, 1, 2] and Thickness(every=7).resolve(3) == [2]


@pytest.mark.parametrize("bad", [[-1], [6], [1.5], [True], ["2"], [None]])
def test_thickness_refuses_bad_indices(bad):
    from pyslice_amd.thickness import as_thickness
    with pytest.raises(ValueError, match="thickness"):
        as_thickness(bad).resolve(6)


def test_thickness_refuses_bad_requests():
    from pyslice_amd.thickness import Thickness, as_thickness
    for kw in (dict(), dict(slices=[1], every=2), dict(every=0), dict(every=2.0), dict(every=True), dict(slices=3),
               dict(slices=[1], patterns="mean")):
        with pytest.raises(ValueError):
            Thickness(**kw)
    for arg in (3, "12", 2.5):
        with pytest.raises(ValueError, match="thickness"):
            as_thickness(arg)


# ------------------------------------------------------------------ 2. the ABI
def test_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name in ("msl_set_layer_reduce", "msl_layer_fetch", "msl_layer_pacbed_reset", "msl_layer_pacbed_add", "msl_layer_pacbed_download",
                 "msl_layer_reduce_bytes"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _native.EXPORTS
    assert re.search(r"#define MSL_ABI_VERSION 3\b", hdr) and _native.ABI_VERSION == 3
    for bit, name in ((_native.LR_DETECT, "DETECT"), (_native.LR_POLAR, "POLAR"), (_native.LR_DIFFRACT, "DIFFRACT"), (_native.LR_PACBED, "PACBED")):
        assert re.search(r"#define MSL_LR_%s %du\b" % (name, bit), hdr)


# ------------------------------------------------------------------ 3. the calculator
class LayerEngine(RecordingEngine):
    """answers layer_fetch with 100 * (layer + 1) + frame slot + column / 1000 for every probe, the pacbed accumulator with the sum of
    those patterns over the probes added since the reset, and the plain reductions like layer 0 of a one-entry series"""

    def _values(self, L, B, count):
        lay = 100.0 * (np.arange(L) + 1.0)
        D, nb, (bx, by) = self._D, getattr(self, "_n_bins", 0), getattr(self, "_bin", (1, 1))
        det = lay[:, None, None, None] + np.arange(count)[None, None, :, None] + np.arange(D)[None, None, None, :] / 1000.0
        pol = lay[:, None, None, None] + np.arange(count)[None, None, :, None] + np.arange(nb)[None, None, None, :] / 1000.0
        pat = (lay * count)[:, None, None, None] + np.zeros((1, 1, self.wx // bx, self.wy // by))
        return (np.broadcast_to(det, (L, B, count, D)).copy(), np.broadcast_to(pol, (L, B, count, nb)).copy(),
                np.broadcast_to(pat, (L, B) + pat.shape[2:]).copy())

    def __getattr__(self, name):
        call = RecordingEngine.__getattr__(self, name)

        def wrapped(*a, **k):
            got = call(*a, **k)
            if name == "set_polar":
                self._n_bins = a[1]
            if name == "set_layer_reduce":
                self._L, self._what, self._bin = len(a[0]) + 1, a[1], tuple(k.get("bin", (1, 1)))
            if name == "propagate_frames":
                self._count = a[1]
            if name == "propagate_frame":
                self._count = 1
            if name == "layer_fetch":
                det, pol, pat = self._values(self._L, k["B"], a[0])
                return (det if self._what & 1 else None, pol if self._what & 2 else None, pat if self._what & 4 else None)
            if name == "layer_pacbed_reset":
                self._acc = 0.0
            if name == "layer_pacbed_add":
                self._acc = self._acc + self._values(self._L, a[0], self._count)[2].sum(axis=1)
            if name == "layer_pacbed":
                return self._acc
            if name == "detect":
                return self._values(1, k["B"], a[1])[0][0]
            if name == "polar_detect":
                return self._values(1, k["B"], a[1])[1][0]
            if name == "diffract":
                self._bin = tuple(k["bin"])
                return self._values(1, k["B"], a[1])[2][0]
            return got
        return wrapped


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def _dets():
    from pyslice_amd import Detector
    return [Detector("bf", outer=20.0), Detector("adf", inner=40.0, outer=120.0, signal="amplitude")]


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", LayerEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)


def test_constructor_refusals_name_thickness():
    from pyslice_amd import Detector, Diffraction, Imaging, PolarDetector, Spectroscopy
    from pyslice_amd.prism import Prism
    dets = _dets()
    with pytest.raises(ValueError, match="thickness"):
        _calc(thickness=[1])                                         # nothing to reduce
    for kw in (dict(layers=[1]), dict(cache=True), dict(stream_tile=4), dict(k_bin=(2, 2))):
        with pytest.raises(ValueError, match="thickness"):
            _calc(thickness=[1], detectors=dets, **kw)
    with pytest.raises((ValueError, NotImplementedError), match="thickness"):
        _calc(thickness=[1], imaging=Imaging())
    with pytest.raises((ValueError, NotImplementedError), match="thickness"):
        _calc(thickness=[1], spectroscopy=Spectroscopy([Detector("bf", outer=10.0)]))
    with pytest.raises(NotImplementedError, match="thickness"):
        _calc(thickness=[1], detectors=dets, prism=Prism(1))
    with pytest.raises(NotImplementedError, match="thickness"):
        _calc(thickness=[1], diffraction=Diffraction(bin=(2, 2), split=True))
    with pytest.raises(ValueError, match="thickness"):
        _calc(thickness=3, detectors=dets)
    from pyslice_amd import Aberrations
    from pyslice_amd.thickness import Thickness
    _calc(thickness=Thickness(every=2), detectors=dets, polar=PolarDetector(outer=40.0), k_window=(16, 16),
          aberrations=Aberrations(defocus=50.0), probe_batch=2, frame_batch=2)
    _calc(thickness=[0], detectors=dets, diffraction=Diffraction(bin=(2, 2)))


def test_setup_refusals_before_device_work(monkeypatch):
    from pyslice_amd import _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("device work before the check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = _calc(thickness=[99], detectors=_dets())
    with pytest.raises(ValueError, match="thickness"):
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    calc = _calc(thickness=[1], detectors=_dets())
    with pytest.raises(NotImplementedError, match="thickness.*ranks"):
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    assert calc._engine is None


def _setup(calc, n_frames=3):
    calc.setup(_trajectory(n_frames), aperture=30.0, voltage_eV=100e3, slice_thickness=0.2, probe_positions=PP)
    return calc


def test_default_is_unchanged(recorder):
    """thickness=None: no new call, the shapes of before"""
    calc = _setup(_calc(detectors=_dets(), probe_batch=2, frame_batch=2))
    res = calc.run_detectors()
    assert res.signals.shape == (5, 3, 2) and res.layer is None and res.thickness is None
    assert not [l for l in format_calls(calc._engine.calls, PP) if l.startswith(("set_layer_reduce", "layer_"))]
    with pytest.raises(ValueError, match="thickness"):
        res.at(-1)


def test_call_order_two_probe_batches_two_frame_batches(recorder):
    """4 probes x 3 frames at probe_batch=2, frame_batch=2: one set_layer_reduce after the detectors, then per frame batch one build and
    per probe batch set_probes, the slice loop and ONE fetch -- no detect call"""
    calc = _calc(detectors=_dets(), thickness=[2, 0], probe_batch=2, frame_batch=2)
    calc.setup(_trajectory(3), aperture=30.0, voltage_eV=100e3, slice_thickness=0.2, probe_positions=PP[:4])
    nz = len(calc._slice_coords)
    assert calc._thickness == [0, 2, nz - 1]
    res = calc.run_detectors()
    lines = format_calls(calc._engine.calls, PP[:4])
    assert [l for l in lines if l.startswith("set_layer_reduce")] == ["set_layer_reduce((0,2), 1, bin=(1,1))"]
    assert lines.index("set_layer_reduce((0,2), 1, bin=(1,1))") > max(i for i, l in enumerate(lines) if l.startswith("set_detectors"))
    assert not [l for l in lines if l.startswith(("detect(", "polar_detect", "diffract", "set_layers"))]
    keep = [l for l in lines if l.startswith(("build_potential", "set_probes", "propagate_frame", "layer_"))]
    na = calc.trajectory.n_atoms
    want = []
    for n in (2, 1):
        want.append(f"build_potentials(f8({n},{na},3), i4({na},), 2)")
        for xy in ("xy[0,1]", "xy[2,3]"):
            want += [f"set_probes(30, {xy})", f"propagate_frames(0, {n})", f"layer_fetch({n}, B=2)"]
    assert keep == want
    assert res.signals.shape == (4, 3, 2, 3)
    for t, slot in enumerate((0, 1, 0)):
        for l in range(3):
            assert np.array_equal(res.signals[:, t, :, l], np.broadcast_to(100.0 * (l + 1) + slot + np.arange(2) / 1000.0, (4, 2)))


def test_detector_result_fields_and_at(recorder):
    from pyslice_amd import STEMData
    from pyslice_amd.potentials import slice_edges
    calc = _setup(_calc(detectors=_dets(), thickness=[1], probe_batch=2, frame_batch=2))
    res = calc.run_detectors()
    nz = len(calc._slice_coords)
    lo, hi = slice_edges(calc._slice_coords)
    assert np.array_equal(res.layer, [1, nz - 1]) and res.layer.dtype == np.int64
    assert np.array_equal(res.thickness, [hi[1] - lo[0], hi[nz - 1] - lo[0]]) and res.thickness[0] < res.thickness[1]
    last = res.at(-1)
    assert type(last) is STEMData and last.layer is None and last.thickness is None and last.signals.shape == (5, 3, 2)
    assert np.array_equal(last.signals, res.signals[..., 1]) and np.array_equal(res.at(0).signals, res.signals[..., 0])
    assert np.array_equal(res.image("adf"), last.image("adf"))                       # the default is the exit
    assert np.array_equal(res.image("adf", layer=0), res.at(0).image("adf"))
    assert not np.array_equal(res.image("adf", layer=0), res.image("adf"))
    with pytest.raises(IndexError):
        res.at(2)


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("with_detectors", [False, True])
def test_polar_shapes_and_defaults(recorder, per_frame, with_detectors):
    from pyslice_amd import Detector, PolarData, PolarDetector
    pol = PolarDetector(outer=60.0, step=20.0, n_azimuthal=2, per_frame=per_frame)
    calc = _setup(_calc(polar=pol, thickness=[0, 1], probe_batch=2, frame_batch=2, detectors=_dets() if with_detectors else None))
    res = calc.run_polar()
    lines = format_calls(calc._engine.calls, PP)
    assert [l for l in lines if l.startswith("set_layer_reduce")] == [f"set_layer_reduce((0,1), {3 if with_detectors else 2}, bin=(1,1))"]
    assert len([l for l in lines if l.startswith("layer_fetch")]) == 6 and not [l for l in lines if l.startswith(("polar_detect", "detect("))]
    assert res.signals.shape == ((5, 3, 3, 2, 3) if per_frame else (5, 3, 2, 3)) and len(res.layer) == 3 and len(res.thickness) == 3
    bins = np.arange(6).reshape(3, 2) / 1000.0
    for l in range(3):
        if per_frame:
            for t, slot in enumerate((0, 1, 0)):
                assert np.array_equal(res.signals[:, t, :, :, l], np.broadcast_to(100.0 * (l + 1) + slot + bins, (5, 3, 2)))
        else:
            assert np.allclose(res.signals[..., l], np.broadcast_to(100.0 * (l + 1) + 1.0 / 3.0 + bins, (5, 3, 2)), rtol=1e-15, atol=0)
    last = res.at(-1)
    assert type(last) is PolarData and last.layer is None and last.signals.shape == res.signals.shape[:-1]
    assert (res.stem is not None) == with_detectors
    if with_detectors:
        assert res.stem.signals.shape == (5, 3, 2, 3) and last.stem.signals.shape == (5, 3, 2) and np.array_equal(res.stem.layer, res.layer)
    assert np.array_equal(res.integrate(0.0, 40.0), last.integrate(0.0, 40.0))
    assert np.array_equal(res.integrate(0.0, 40.0, layer=0), res.at(0).integrate(0.0, 40.0))
    assert np.array_equal(res.profile(), last.profile()) and np.array_equal(res.profile(1, layer=1), res.at(1).profile(1))
    assert np.array_equal(res.image(0.0, 20.0), last.image(0.0, 20.0))
    if per_frame:
        d = [Detector("v", inner=20.0, outer=60.0)]
        assert np.array_equal(res.to_stem(d).signals, last.to_stem(d).signals)
        assert np.array_equal(res.to_stem(d, layer=0).signals, res.at(0).to_stem(d).signals)


@pytest.mark.parametrize("with_detectors", [False, True])
def test_diffraction_position_shapes_and_defaults(recorder, with_detectors):
    from pyslice_amd import Detector, Diffraction, DiffractionData
    calc = _setup(_calc(diffraction=Diffraction(bin=(4, 2)), thickness=[1], probe_batch=2, frame_batch=2,
                        detectors=_dets() if with_detectors else None))
    res = calc.run_diffraction()
    lines = format_calls(calc._engine.calls, PP)
    assert [l for l in lines if l.startswith("set_layer_reduce")] == [f"set_layer_reduce((1), {5 if with_detectors else 4}, bin=(4,2))"]
    assert not [l for l in lines if l.startswith(("diffract", "detect(", "layer_pacbed"))]
    assert res.intensity.shape == (5, 8, 16, 2) and res.patterns == "position"
    for l in range(2):                                               # sum over 2 + 1 frames of 100 (l + 1) per frame, / 3
        assert np.allclose(res.intensity[..., l], 100.0 * (l + 1), rtol=1e-15, atol=0)
    last = res.at(-1)
    assert type(last) is DiffractionData and last.layer is None and last.intensity.shape == (5, 8, 16)
    assert (res.stem is not None) == with_detectors
    if with_detectors:
        assert res.stem.signals.shape == (5, 3, 2, 2) and last.stem.signals.shape == (5, 3, 2)
    v = Detector("v", inner=10.0, outer=80.0)
    assert np.array_equal(res.pacbed(), last.pacbed()) and np.array_equal(res.pacbed(layer=0), res.at(0).pacbed())
    assert np.array_equal(res.virtual(v), last.virtual(v)) and np.array_equal(res.virtual(v, layer=0), res.at(0).virtual(v))
    assert np.array_equal(res.image(v), last.image(v)) and np.array_equal(res.image(v, layer=0), res.at(0).image(v))
    assert np.array_equal(res.pattern(0.3, 0.2), last.pattern(0.3, 0.2))
    assert np.array_equal(res.pattern(0.3, 0.2, layer=0), res.at(0).pattern(0.3, 0.2))


def test_diffraction_pacbed_mode(recorder):
    """patterns="pacbed": per frame batch reset, one add per probe batch, one download; (mx, my, L), divided by P * T"""
    from pyslice_amd import Detector, Diffraction
    from pyslice_amd.thickness import Thickness
    calc = _setup(_calc(diffraction=Diffraction(bin=(4, 2)), thickness=Thickness(slices=[1], patterns="pacbed"), probe_batch=2, frame_batch=2))
    res = calc.run_diffraction()
    lines = format_calls(calc._engine.calls, PP)
    assert [l for l in lines if l.startswith("set_layer_reduce")] == ["set_layer_reduce((1), 8, bin=(4,2))"]
    keep = [l for l in lines if l.startswith(("propagate_frame", "layer_"))]
    want = []
    for n in (2, 1):
        for i, real in enumerate((2, 2, 1)):
            want += [f"propagate_frames(0, {n})"] + (["layer_pacbed_reset()"] if i == 0 else []) + [f"layer_pacbed_add({real})"]
        want.append("layer_pacbed()")
    assert keep == want                                              # (no fetch: nothing but the accumulator is wanted)
    assert res.intensity.shape == (8, 16, 2) and res.patterns == "pacbed"
    for l in range(2):                                               # 5 probes x 3 frames of 100 (l + 1), / (P T)
        assert np.allclose(res.intensity[..., l], 100.0 * (l + 1), rtol=1e-15, atol=0)
    assert res.at(-1).intensity.shape == (8, 16) and np.array_equal(res.pacbed(), res.intensity[..., -1])
    assert np.array_equal(res.pacbed(layer=0), res.intensity[..., 0])
    with pytest.raises(ValueError, match="pacbed"):
        res.virtual(Detector("v", inner=10.0, outer=80.0))
    with pytest.raises(ValueError, match="pacbed"):
        res.pattern(0.0, 0.0)


def test_exit_only_series_takes_the_plain_reductions(recorder):
    """a series whose only entry is the exit wave has no tap: no reduce mode, the plain calls, a thickness axis of one"""
    from pyslice_amd import Diffraction
    from pyslice_amd.thickness import Thickness
    calc = _setup(_calc(diffraction=Diffraction(bin=(4, 2)), detectors=_dets(), thickness=Thickness(every=1000, patterns="pacbed"),
                        probe_batch=2, frame_batch=2))
    res = calc.run_diffraction()
    lines = format_calls(calc._engine.calls, PP)
    assert not [l for l in lines if l.startswith(("set_layer_reduce", "layer_"))]
    assert len([l for l in lines if l.startswith("diffract")]) == 6 and len([l for l in lines if l.startswith("detect(")]) == 6
    assert res.intensity.shape == (8, 16, 1) and res.stem.signals.shape == (5, 3, 2, 1) and len(res.layer) == 1
    assert np.allclose(res.intensity[..., 0], 100.0, rtol=1e-15, atol=0)


def test_staging_is_counted_in_the_probe_batch(monkeypatch):
    """the automatic probe batch shrinks when the block, the tap buffer and the staging of the entries are added"""
    from pyslice_amd import Diffraction, _native, calculators
    monkeypatch.setattr(_native, "Engine", LayerEngine)
    got = {}
    for name, th in (("plain", None), ("series", list(range(0, 4)))):
        calc = _calc(diffraction=Diffraction(bin=(1, 1)), thickness=th)
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, slice_thickness=0.2, probe_positions=PP * 60)
        nx, ny, nz = calc.nx, calc.ny, len(calc._slice_coords)
        plain_need = 256 * (32.0 * nx * ny + 8.0 * nx * ny) + 16.0 * nz * nx * ny + calc._phase_table_bytes(1) + 1e9
        monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: (plain_need + 1e5) / 0.9)
        calc.setup(_trajectory(1), aperture=30.0, voltage_eV=100e3, slice_thickness=0.2, probe_positions=PP * 60)
        got[name] = calc.probe_batch
        monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    assert got["plain"] == 256 and got["series"] < 256


def test_series_that_does_not_fit_is_retried_at_a_smaller_probe_batch(monkeypatch):
    """the block, the tap buffer and the staging are allocated inside the shrink-and-retry of the engine: MemoryError from
    set_layer_reduce at an automatic probe batch halves it, on a fresh engine with the whole set-up made again"""
    from pyslice_amd import _native, calculators
    made = []

    class TightEngine(LayerEngine):
        def __init__(self, *a, **k):
            LayerEngine.__init__(self, *a, **k)
            made.append(self)

        def __getattr__(self, name):
            call = LayerEngine.__getattr__(self, name)
            if name != "set_layer_reduce":
                return call

            def set_layer_reduce(*a, **k):
                if self.n_probes > 2:
                    raise MemoryError("msl_set_layer_reduce: does not fit")
                return call(*a, **k)
            return set_layer_reduce
    monkeypatch.setattr(_native, "Engine", TightEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    calc = _setup(_calc(detectors=_dets(), thickness=[1], frame_batch=2))
    assert [e.n_probes for e in made] == [5, 2] and calc.probe_batch == 2 and calc._engine is made[1]
    assert [l for l in format_calls(made[0].calls) if l.startswith("close")] == ["close()"]
    lines = format_calls(made[1].calls, PP)
    assert [l.split("(")[0] for l in lines][:5] == ["set_kirkland", "set_slices", "set_aberrations", "set_detectors", "set_layer_reduce"]
    assert calc.run_detectors().signals.shape == (5, 3, 2, 2)
    monkeypatch.setattr(_native, "Engine", type("Explicit", (TightEngine,), {}))
    with pytest.raises(MemoryError):                                 # an explicit probe batch is honoured as is
        _setup(_calc(detectors=_dets(), thickness=[1], probe_batch=4, frame_batch=2))


# ------------------------------------------------------------------ 4. the layout of the staging area (no device)
def test_layout_check_program_builds_and_passes(tmp_path):
    """tools/layer_reduce_layout_check.cpp: the offsets of every section and layer against a brute-force walk"""
    import shutil
    import subprocess
    from pyslice_amd import build_native
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(build_native._hipcc())), "..", "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler, not even the ROCm clang++ the library is built with"
    exe = tmp_path / "layout_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", str(exe), os.path.join(REPO, "tools", "layer_reduce_layout_check.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "FAILED" not in out and "all ok" in out
