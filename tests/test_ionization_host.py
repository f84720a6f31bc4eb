"""Element maps on the host: the float64 definition (pyslice_amd/ionization.py) -- the sum rules of the weights and of the slice loop,
periodic wrapping, absent elements, two widths of one element --, the Ionization argument, the calculator's refusals and calls (a
RecordingEngine subclass: no device), the result type, and the C ABI's bindings."""
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV = 100e3
NX, NY, NZ, D, DZ = 48, 40, 4, 0.1, 1.0


def grid():
    xs, ys = np.arange(NX) * D, np.arange(NY) * D
    zs = (np.arange(NZ) + 0.5) * DZ
    return xs, ys, zs


def atoms(seed=0, n=14):
    """Si and O anywhere in the cell: slices of 1 A, the last one up to 4.5 A (slice_edges)"""
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 3)) * np.array([NX * D, NY * D, NZ * DZ])
    Z = np.array([14, 8] * (n // 2), dtype=np.int32)
    return pos, Z


def channels():
    from pyslice_amd.ionization import Ionization
    return [Ionization(14, 0.15, 0.7), Ionization("O", 0.4, 1.3), Ionization(14, 0.4, 0.7, name="Si-L"), Ionization(79, 0.3)]


def propagator():
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.tilt import tilted_propagator
    return tilted_propagator(NX, NY, D, D, wavelength(EV), DZ, None)


# ---- the weights -------------------------------------------------------------------------------------------
def test_weights_integrate_to_cross_section_times_atoms_per_slice():
    from pyslice_amd.ionization import ionization_weights
    from pyslice_amd.potentials import slice_edges
    xs, ys, zs = grid()
    pos, Z = atoms()
    W = ionization_weights(channels(), xs, ys, zs, pos, Z)
    assert W.shape == (4, NZ, NX, NY)
    lo, hi = slice_edges(zs)
    for e, ch in enumerate(channels()):
        for s in range(NZ):
            n = int(((Z == ch.Z) & (pos[:, 2] >= lo[s]) & (pos[:, 2] < hi[s])).sum())
            assert abs(W[e, s].sum() * D * D - ch.cross_section * n) <= 1e-12 * max(1.0, ch.cross_section * n)
    assert not W[3].any()                                       # no gold in the cell: zeros, not an error


def test_plane_wave_on_the_first_slice_gives_n_c_over_area():
    from pyslice_amd.ionization import ionization_signal, ionization_weights
    from pyslice_amd.potentials import slice_edges
    xs, ys, zs = grid()
    pos, Z = atoms(1)
    chs = channels()
    W = ionization_weights(chs, xs, ys, zs, pos, Z)
    rng = np.random.default_rng(5)
    t = np.exp(1j * rng.random((NZ, NX, NY)))
    I, _ = ionization_signal(np.full((1, NX, NY), 0.3 + 0.4j), t, W, propagator())
    lo, hi = slice_edges(zs)
    area = NX * D * NY * D
    for e, ch in enumerate(chs):
        n = int(((Z == ch.Z) & (pos[:, 2] >= lo[0]) & (pos[:, 2] < hi[0])).sum())
        assert abs(I[0, e, 0] - n * ch.cross_section / area) <= 1e-12


def test_vacuum_total_is_n_c_over_area_for_any_placement():
    from pyslice_amd.ionization import ionization_signal, ionization_weights
    xs, ys, zs = grid()
    area = NX * D * NY * D
    chs = channels()
    for seed in (2, 3):
        pos, Z = atoms(seed)
        W = ionization_weights(chs, xs, ys, zs, pos, Z)
        I, ex = ionization_signal(np.ones((1, NX, NY)), np.ones((NZ, NX, NY), dtype=complex), W, propagator())
        for e, ch in enumerate(chs):
            assert abs(I[0, e].sum() - int((Z == ch.Z).sum()) * ch.cross_section / area) <= 1e-12
        assert np.abs(ex - 1.0).max() <= 1e-12


def test_a_gaussian_on_the_cell_edge_wraps_periodically():
    from pyslice_amd.ionization import Ionization, ionization_weights
    xs, ys, zs = grid()
    ch = [Ionization(14, 0.3, 2.0)]
    edge = ionization_weights(ch, xs, ys, zs, np.array([[0.0, 1.2, 0.5]]), [14])[0, 0]
    mid = ionization_weights(ch, xs, ys, zs, np.array([[10 * D, 1.2, 0.5]]), [14])[0, 0]
    assert np.abs(np.roll(mid, -10, axis=0) - edge).max() <= 1e-12 * mid.max()
    assert edge[-1, 12] > 0.5 * edge[0, 12] and abs(edge[-1, 12] - edge[1, 12]) <= 1e-12 * edge.max()      # both sides of the edge
    # the peak is the Gaussian's: c / (2 pi w^2), the neighbouring cells' tails are below 1e-12 of it at this width
    assert abs(edge[0, 12] - 2.0 / (2.0 * np.pi * 0.09)) <= 1e-9 * edge[0, 12]


def test_two_widths_of_one_element_give_different_signals():
    from pyslice_amd.ionization import ionization_signal, ionization_weights
    xs, ys, zs = grid()
    pos, Z = atoms(4)
    W = ionization_weights(channels(), xs, ys, zs, pos, Z)
    x, y = np.meshgrid(xs, ys, indexing="ij")
    probe = np.exp(-((x - pos[0, 0]) ** 2 + (y - pos[0, 1]) ** 2) / (2 * 0.25 ** 2)).astype(complex)[None]
    I, _ = ionization_signal(probe, np.ones((NZ, NX, NY), dtype=complex), W, propagator())
    assert I.shape == (1, 4, NZ)
    assert np.abs(I[0, 0] - I[0, 2]).max() > 0.05 * np.abs(I[0, 0]).max()
    assert not I[0, 3].any()
    with pytest.raises(ValueError, match="weights"):
        ionization_signal(probe, np.ones((NZ, NX, NY), dtype=complex), W[:, :2], propagator())


# ---- the argument ------------------------------------------------------------------------------------------
def test_ionization_validation():
    from pyslice_amd.ionization import Ionization, check_ionization
    a = Ionization("Si", 0.2)
    assert (a.Z, a.width, a.cross_section, a.name) == (14, 0.2, 1.0, "Si")
    assert Ionization(8, 0.1, 0.0, name="O-K").name == "O-K"
    for bad in (dict(element="Xx", width=0.1), dict(element=0, width=0.1), dict(element=104, width=0.1), dict(element=1.5, width=0.1),
                dict(element=14, width=0.0), dict(element=14, width=-1.0), dict(element=14, width=np.inf), dict(element=14, width=np.nan),
                dict(element=14, width=0.1, cross_section=-1e-9), dict(element=14, width=0.1, cross_section=np.nan),
                dict(element=14, width="wide")):
        with pytest.raises(ValueError, match="Ionization"):
            Ionization(**bad)
    assert len(check_ionization([a] * 8)) == 8 and check_ionization(a) == [a]
    for bad in ([], [a] * 9, [a, (14, 0.1, 1.0)], 3):
        with pytest.raises(ValueError, match="ionization"):
            check_ionization(bad)


# ---- the calculator ----------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (2.8, 0.4), (0.5, 0.5)]


@pytest.fixture(scope="module")
def source():
    import pyslice_amd as ps
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(NX, NZ, D, DZ, NY)
    pos, Z = atoms(6, 12)
    return ps.Trajectory(Z, np.stack([pos, pos + 0.01]), np.zeros((2, 12, 3)), box, 0.005)


def _calc(**kw):
    import pyslice_amd as ps
    return ps.MultisliceCalculator(device=0, progress=False, **kw)


def _setup(calc, src):
    calc.setup(src, aperture=30.0, voltage_eV=EV, probe_positions=PP, sampling=D, slice_thickness=DZ)


def test_refusals_come_before_any_device_work(source, monkeypatch):
    from pyslice_amd import _native, distributed
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.imaging import Imaging
    from pyslice_amd.polar_data import PolarDetector
    from pyslice_amd.prism import Prism
    from pyslice_amd.spectroscopy import Spectroscopy
    from pyslice_amd.stem_data import Detector
    from pyslice_amd.tilt import Precession

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the refusal")
    monkeypatch.setattr(_native, "Engine", no_engine)
    dets = [Detector("d", inner=30.0, outer=70.0)]
    refused = dict(tds=dict(tds=True, detectors=dets), prism=dict(prism=Prism(1)), precession=dict(precession=Precession(10.0, 4)),
                   projection=dict(projection="finite"), detectors=dict(detectors=dets),
                   polar=dict(polar=PolarDetector(outer=100.0, step=10.0)), diffraction=dict(diffraction=Diffraction()),
                   imaging=dict(imaging=Imaging()), spectroscopy=dict(spectroscopy=Spectroscopy(detectors=dets)),
                   layers=dict(layers=[0]), thickness=dict(thickness=[0, 2]), k_window=dict(k_window=(16, 16)), k_bin=dict(k_bin=(2, 2)),
                   cache=dict(cache=True), stream_tile=dict(stream_tile=2), frame_batch=dict(frame_batch=2))
    for what, kw in refused.items():
        with pytest.raises(NotImplementedError, match=rf"ionization: {what}.* is not built"):
            _calc(ionization=channels(), **kw)
    for bad in ([], channels() * 3, [(14, 0.1, 1.0)]):
        with pytest.raises(ValueError, match="ionization"):
            _calc(ionization=bad)
    _calc(ionization=channels(), frame_batch=1)                 # (a frame batch of one is what the run uses)
    with pytest.raises(RuntimeError, match="run_element_maps\\(\\) needs"):
        _calc().run_element_maps()
    with pytest.raises(RuntimeError, match="call setup"):
        _calc(ionization=channels()).run_element_maps()
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="ionization: a run over several ranks is not built"):
        _setup(_calc(ionization=channels()), source)


class IonEngine(RecordingEngine):
    """RecordingEngine with the engine methods of this feature spelled out: ionization_fetch answers (nz, B, E) with
    100 * (call number) + 10 * slice + channel + probe / 10"""

    def __init__(self, nx, ny, nz, *a, **k):
        super().__init__(nx, ny, nz, *a, **k)
        self.nz, self.n_ionization, self._fetches = nz, 0, 0

    def set_ionization(self, channels=None):
        self.calls.append(("set_ionization", (list(channels or []),), {}))
        self.n_ionization = len(channels or [])

    def ionization_fetch(self, B=None):
        self.calls.append(("ionization_fetch", (), dict(B=B)))
        self._fetches += 1
        s, p, e = np.meshgrid(np.arange(self.nz), np.arange(B), np.arange(self.n_ionization), indexing="ij")
        return 100.0 * self._fetches + 10.0 * s + e + p / 10.0


def test_run_sets_the_channels_before_the_build_and_adds_every_frame(source, monkeypatch):
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    monkeypatch.setattr(_native, "Engine", IonEngine)
    calc = _calc(ionization=channels(), probe_batch=2)
    _setup(calc, source)
    eng = calc._engine
    assert (eng.n_probes, eng.frame_batch, eng.n_frames) == (2, 1, 1)
    res = calc.run_element_maps()
    names = [c[0] for c in eng.calls]
    assert names.count("set_ionization") == 1 and names.index("set_ionization") < names.index("build_potential")
    assert eng.calls[names.index("set_ionization")][1][0] == channels()
    # two frames x two probe batches: one build per frame, one loop and one fetch per batch, the padded batch fetched short
    assert names.count("build_potential") == 2 and names.count("propagate_frame") == 4
    assert [c[2]["B"] for c in eng.calls if c[0] == "ionization_fetch"] == [2, 1, 2, 1]
    assert not any(n in names for n in ("set_tds", "set_detectors", "detect", "build_potentials", "propagate_frames"))
    # the mean over the frames of what the fetches returned: fetches 1, 2 are frame 0, fetches 3, 4 frame 1
    assert res.per_slice.shape == (3, 4, NZ)
    s, e = np.meshgrid(np.arange(NZ), np.arange(4), indexing="ij")
    for p, (first, row) in enumerate([(1, 0), (1, 1), (2, 0)]):
        want = 0.5 * ((100.0 * first + 10.0 * s + e + row / 10.0) + (100.0 * (first + 2) + 10.0 * s + e + row / 10.0))
        assert np.array_equal(res.per_slice[p], want.T)
    lo, hi = slice_edges(calc._slice_coords)
    assert np.array_equal(res.thickness, hi - lo[0]) and res.names == ["Si", "O", "Si-L", "Au"] and res.n_frames == 2
    assert res.probe_positions == PP
    with pytest.raises(RuntimeError, match="call run_element_maps"):
        calc.run()


def test_without_ionization_the_calculator_makes_todays_calls(source, monkeypatch):
    from pyslice_amd import _native
    from pyslice_amd.stem_data import Detector
    monkeypatch.setattr(_native, "Engine", IonEngine)
    seqs = []
    for kw in ({}, dict(ionization=None)):
        calc = _calc(detectors=[Detector("d", inner=30.0, outer=70.0)], probe_batch=2, **kw)
        _setup(calc, source)
        calc.run_detectors()
        seqs.append(format_calls(calc._engine.calls, PP))
        assert calc._ionization is None
    assert seqs[0] == seqs[1] and not any("ionization" in line for line in seqs[0])


def test_probe_batch_fit_counts_the_weight_stack(source, monkeypatch):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", IonEngine)
    got = []
    for n in (1, 8):
        calc = _calc(ionization=channels()[:1] * n)
        _setup(calc, source)
        # free memory such that the run with one channel just keeps 256 probes: the seven further stacks must cost some of them
        calc.n_probes = 256
        npix = calc.nx * calc.ny
        free = (256 * (32.0 * npix + 8.0 * calc._stored_shape()[2]) + calc._stack_bytes() * calc.nz * npix + calc._phase_table_bytes(1)
                + 4.0 * (calc.nz + 8) * npix + 1e9) / 0.9 + 1.0
        got.append(calc._fit_probe_batch(free, 256, 1))
    assert got[0] == 256 and got[1] < 256


# ---- the result --------------------------------------------------------------------------------------------
def test_element_map_data_accessors():
    from pyslice_amd.element_map_data import ElementMapData
    rng = np.random.default_rng(9)
    pp = [(x, y) for x in (0.0, 1.0, 2.0) for y in (0.0, 1.0)]
    per = rng.random((6, 2, 5))
    chs = channels()[:2]
    res = ElementMapData(per_slice=per, channels=chs, probe_positions=pp, thickness=np.arange(1, 6) * 0.5, n_frames=3)
    assert res.names == ["Si", "O"]
    assert res.signals.shape == (6, 2) and np.array_equal(res.cumulative()[..., -1], res.signals)
    assert np.abs(res.signals - per.sum(axis=-1)).max() <= 1e-15 * 5
    assert res.cumulative().shape == (6, 2, 5) and np.array_equal(res.cumulative()[..., 0], per[..., 0])
    img = res.image("O")
    assert img.shape == (3, 2) and np.array_equal(img, res.signals[:, 1].reshape(3, 2))
    assert np.array_equal(res.image("O", slice=2), res.cumulative()[:, 1, 2].reshape(3, 2))
    assert np.array_equal(res.image("Si", slice=-1), res.image("Si")) and np.array_equal(res.image(0), res.image("Si"))
    assert np.array_equal(res.depth_profile("Si", 4), per[4, 0])
    with pytest.raises(KeyError):
        res.image("Au")
    with pytest.raises(IndexError):
        res.image("O", slice=5)
    with pytest.raises(ValueError, match="per_slice"):
        ElementMapData(per_slice=per[:, :1], channels=chs, probe_positions=pp, thickness=np.arange(5))


# ---- the C ABI ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_exports():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name in ("msl_set_ionization", "msl_ionization_fetch", "msl_ionization_reduce"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr) and name in _native.EXPORTS
    assert re.search(r"MSL_BUF_IONIZATION_WEIGHT = 18\b", hdr) and _native.BUF_IONIZATION_WEIGHT == 18
    assert _native.IONIZATION_MAX_CHANNELS == 8
