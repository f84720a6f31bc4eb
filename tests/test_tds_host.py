"""TDS detector signal of the absorptive potential on the host: the float64 definition (pyslice_amd/tds.py) -- its tables against
absorptive_tables, linearity in the detector, conservation of the slice loop --, the calculator's refusals and calls (a RecordingEngine
subclass: no device), the result type, and the C ABI's bindings."""
import os
import re

import numpy as np
import pytest

from oracle import multislice_oracle as orc
from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV = 100e3
U = {14: 0.078, 8: 0.09}


def annulus(q, lo, hi):
    return (q >= lo) & (q < hi)


@pytest.fixture(scope="module")
def grid():
    """48 x 40 pixels of 0.1 A: q2, |q| and the form-factor tables of Si and O on the fftfreq grid"""
    nx, ny, dx, dy = 48, 40, 0.1, 0.1
    q2 = np.fft.fftfreq(nx, dx)[:, None] ** 2 + np.fft.fftfreq(ny, dy)[None, :] ** 2
    out = dict(nx=nx, ny=ny, dx=dx, dy=dy, q2=q2, q=np.sqrt(q2), f={Z: orc.form_factor(q2, Z) for Z in U})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the tables --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", [14, 8])
def test_whole_plane_detector_gives_the_absorptive_table(grid, Z):
    from pyslice_amd.absorptive import absorptive_tables
    from pyslice_amd.tds import tds_tables
    g = absorptive_tables(grid["f"][Z], grid["q2"], U[Z], grid["dx"], grid["dy"])[1]
    got = tds_tables(grid["f"][Z], grid["q2"], U[Z], grid["dx"], grid["dy"], np.ones(g.shape, dtype=bool))
    assert np.abs(got - g).max() <= 1e-12 * np.abs(g).max()


@pytest.mark.parametrize("Z", [14, 8])
def test_a_partition_of_the_plane_sums_to_the_absorptive_table(grid, Z):
    from pyslice_amd.absorptive import absorptive_tables
    from pyslice_amd.tds import tds_tables
    g = absorptive_tables(grid["f"][Z], grid["q2"], U[Z], grid["dx"], grid["dy"])[1]
    q = grid["q"]
    parts = [annulus(q, 0.0, 1.2), annulus(q, 1.2, 3.1), annulus(q, 3.1, np.inf)]
    assert all(p.any() for p in parts) and np.array_equal(sum(p.astype(int) for p in parts), np.ones(q.shape, dtype=int))
    tabs = [tds_tables(grid["f"][Z], grid["q2"], U[Z], grid["dx"], grid["dy"], p) for p in parts]
    assert np.abs(sum(tabs) - g).max() <= 1e-12 * np.abs(g).max()
    assert all(np.abs(t).max() > 1e-6 * np.abs(g).max() for t in tabs)          # (every annulus carries some of it)


def test_no_vibration_no_tds(grid):
    from pyslice_amd.tds import tds_tables, tds_weight
    got = tds_tables(grid["f"][14], grid["q2"], 0.0, grid["dx"], grid["dy"], annulus(grid["q"], 1.0, 3.0))
    assert got.shape == grid["q2"].shape and not got.any()
    assert not tds_weight(got, orc.interaction_sigma(EV)).any()
    with pytest.raises(ValueError, match="membership"):
        tds_tables(grid["f"][14], grid["q2"], 0.1, grid["dx"], grid["dy"], np.ones((3, 3)))


# ---- the slice loop ----------------------------------------------------------------------------------------
def stack_from_tables(xs, ys, zs, pos, Z, tables):
    """(nz, nx, ny) float64: the structure-factor sum of every slice with tables[Z] in the place of the form factor, inverse
    transformed, over 1 / (dx^2 dy^2) -- the way absorptive.py says Vbar and Omega are built"""
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    lo, hi = orc.slice_edges(zs)
    kxs, kys = np.fft.fftfreq(len(xs), d=dx), np.fft.fftfreq(len(ys), d=dy)
    recip = np.zeros((len(zs), len(xs), len(ys)), dtype=np.complex128)
    for z in np.unique(Z):
        sel = pos[Z == z]
        for s in range(len(zs)):
            m = (sel[:, 2] >= lo[s]) & (sel[:, 2] < hi[s])
            if m.any():
                recip[s] += (np.exp(-2j * np.pi * np.outer(kxs, sel[m, 0])) @ np.exp(-2j * np.pi * np.outer(sel[m, 1], kys))) * tables[int(z)]
    return np.fft.ifft2(recip, axes=(1, 2)).real / (dx ** 2 * dy ** 2)


def test_whole_plane_detector_conserves_the_electrons():
    """48 x 40 x 3, two probes: sum |psi_exit|^2 + sum_s I_s = sum |psi_0|^2 to 1e-12, and two half planes share the same sum"""
    import pyslice_amd as ps
    from pyslice_amd.absorptive import absorptive_tables, absorptive_transmission
    from pyslice_amd.synthetic import box_for_grid
    from pyslice_amd.tds import tds_signal, tds_tables, tds_weight
    from pyslice_amd.tilt import tilted_propagator
    nx, ny, nz = 48, 40, 3
    box = box_for_grid(nx, nz, 0.1, 1.0, ny)
    rng = np.random.default_rng(7)
    pos = rng.random((30 * nz, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    Z = np.array([14, 8], dtype=np.int32)[rng.integers(0, 2, len(pos))]
    ap = ps.AbsorptivePotential(Z, pos, box, U)
    xs, ys, zs = ps.gridFromTrajectory(ap, 0.1, 1.0)[:3]
    assert (len(xs), len(ys), len(zs)) == (nx, ny, nz)
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    q2 = np.fft.fftfreq(nx, dx)[:, None] ** 2 + np.fft.fftfreq(ny, dy)[None, :] ** 2
    sigma = orc.interaction_sigma(EV)
    f = {z: orc.form_factor(q2, z) for z in U}
    tabs = {z: absorptive_tables(f[z], q2, U[z], dx, dy) for z in U}
    Vbar = stack_from_tables(xs, ys, zs, pos, Z, {z: tabs[z][0] for z in U})
    Om = stack_from_tables(xs, ys, zs, pos, Z, {z: tabs[z][1] for z in U})
    t = absorptive_transmission(Vbar, Om, sigma)
    upper = np.sqrt(q2) >= 2.0
    members = [np.ones(q2.shape, dtype=bool), upper, ~upper]
    w = np.stack([tds_weight(stack_from_tables(xs, ys, zs, pos, Z, {z: tds_tables(f[z], q2, U[z], dx, dy, M) for z in U}), sigma)
                  for M in members])
    probes = orc.batched_probes(orc.probe_array(xs, ys, 30.0, EV), xs, ys, [(1.3, 2.05), (2.8, 0.4)])
    prop = tilted_propagator(nx, ny, dx, dy, orc.wavelength(EV), zs[1] - zs[0], None)
    assert np.abs(np.abs(prop) - 1.0).max() <= 1e-14
    I, ex = tds_signal(probes, t, w, prop)
    assert I.shape == (2, 3, nz) and ex.shape == probes.shape
    n0, n1 = (np.abs(probes) ** 2).sum(axis=(1, 2)), (np.abs(ex) ** 2).sum(axis=(1, 2))
    assert np.abs((n1 + I[:, 0].sum(axis=1)) / n0 - 1.0).max() <= 1e-12
    assert (I[:, 0].sum(axis=1) > 1e-4 * n0).all()              # (something was absorbed)
    # the two halves are the whole only to first order in sigma^2 Omega: w is not linear in Omega_det
    assert np.abs((I[:, 1] + I[:, 2]) / I[:, 0] - 1.0).max() <= 0.05
    with pytest.raises(ValueError, match="weight"):
        tds_signal(probes, t, w[:, :2], prop)


# ---- the calculator ----------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (2.8, 0.4), (0.5, 0.5)]


@pytest.fixture(scope="module")
def source():
    from pyslice_amd.absorptive import AbsorptivePotential
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(48, 3, 0.1, 1.0, 40)
    rng = np.random.default_rng(3)
    pos = rng.random((12, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    return AbsorptivePotential(np.array([14, 8] * 6, dtype=np.int32), pos, box, U)


def dets(n=2):
    from pyslice_amd.stem_data import Detector
    return [Detector(f"d{i}", inner=30.0 + 40.0 * i, outer=70.0 + 40.0 * i) for i in range(n)]


def _calc(**kw):
    import pyslice_amd as ps
    return ps.MultisliceCalculator(device=0, progress=False, **kw)


def _setup(calc, src):
    calc.setup(src, aperture=30.0, voltage_eV=EV, probe_positions=PP, sampling=0.1, slice_thickness=1.0)


def test_refusals_come_before_any_device_work(source, monkeypatch):
    from pyslice_amd import _native, distributed
    from pyslice_amd.absorptive import AbsorptivePotential
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
    with pytest.raises(ValueError, match="tds=True needs detectors"):
        _calc(tds=True)
    with pytest.raises(NotImplementedError, match="tds: more than 4 detectors is not built"):
        _calc(tds=True, detectors=dets(5))
    with pytest.raises(NotImplementedError, match="tds: a segmented detector .* is not built"):
        _calc(tds=True, detectors=[Detector("seg", inner=30.0, outer=60.0, azimuth=(0.0, 90.0))])
    for sig in ("amplitude", "com_x", "com_y"):
        with pytest.raises(NotImplementedError, match="tds: the signal .* is not built"):
            _calc(tds=True, detectors=[Detector("a", inner=30.0, outer=60.0, signal=sig)])
    for kw in (dict(prism=Prism(1)), dict(precession=Precession(10.0, 4)), dict(polar=PolarDetector(outer=100.0, step=10.0)),
               dict(diffraction=Diffraction())):
        with pytest.raises(NotImplementedError, match=r"tds: .* is not built"):
            _calc(tds=True, detectors=dets(), **kw)
    # what detectors= itself refuses stays refused, by its own message, before tds is looked at
    for kw in (dict(layers=[0]), dict(cache=True), dict(stream_tile=2), dict(imaging=Imaging()),
               dict(spectroscopy=Spectroscopy(detectors=dets(1)))):
        with pytest.raises((ValueError, NotImplementedError)):
            _calc(tds=True, detectors=dets(), **kw)
    # the potential: setup() is the first to see it
    for bad in (source.frozen_phonons(1).to_trajectory(),
                AbsorptivePotential(source.atom_types, source.base_positions, source.box_matrix, U, absorption=False)):
        with pytest.raises(ValueError, match="tds=True needs an absorptive.AbsorptivePotential"):
            _setup(_calc(tds=True, detectors=dets()), bad)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="is not built"):
        _setup(_calc(tds=True, detectors=dets()), source)


class TdsEngine(RecordingEngine):
    """RecordingEngine with the engine methods of this feature spelled out: tds_fetch answers (nz, B, D) with
    100 * (call number) + 10 * slice + detector + probe / 10, layer_fetch with zeros"""

    def __init__(self, nx, ny, nz, *a, **k):
        super().__init__(nx, ny, nz, *a, **k)
        self.nz, self.n_tds, self._fetches, self._layers_n = nz, 0, 0, 0

    def set_absorption(self, u_by_Z=None, absorb=True):
        self.calls.append(("set_absorption", (None if u_by_Z is None else np.array(u_by_Z), absorb), {}))

    def set_tds(self, member_bits=None, n_det=0):
        self.calls.append(("set_tds", (None if member_bits is None else np.array(member_bits), n_det), {}))
        self.n_tds = n_det

    def set_layer_reduce(self, slices, what, bin=(1, 1)):
        self.calls.append(("set_layer_reduce", (list(slices), what), dict(bin=bin)))
        self._layers_n = len(slices) + 1

    def layer_fetch(self, count, B=None):
        self.calls.append(("layer_fetch", (count,), dict(B=B)))
        return np.zeros((self._layers_n, B, count, self._D)), None, None

    def tds_fetch(self, B=None):
        self.calls.append(("tds_fetch", (), dict(B=B)))
        self._fetches += 1
        s, p, d = np.meshgrid(np.arange(self.nz), np.arange(B), np.arange(self.n_tds), indexing="ij")
        return 100.0 * self._fetches + 10.0 * s + d + p / 10.0


def test_tds_run_sets_the_detectors_before_the_build_and_fetches_every_batch(source, monkeypatch):
    from pyslice_amd import _native
    from pyslice_amd.stem_data import Detector
    from pyslice_amd.tds import tds_members
    monkeypatch.setattr(_native, "Engine", TdsEngine)
    calc = _calc(tds=True, detectors=dets(2), probe_batch=2)
    _setup(calc, source)
    res = calc.run_detectors()
    names = [c[0] for c in calc._engine.calls]
    assert names.count("set_tds") == 1
    assert names.index("set_absorption") < names.index("set_tds") < names.index("build_potential")
    bits, n = calc._engine.calls[names.index("set_tds")][1]
    assert n == 2 and bits.shape == (calc.nx, calc.ny) and bits.dtype == np.uint16
    lam = orc.wavelength(EV)
    assert np.array_equal(bits, tds_members(dets(2), calc.nx, calc.ny, calc.dx, calc.dy, lam))
    q = np.hypot(np.fft.fftfreq(calc.nx, calc.dx)[:, None], np.fft.fftfreq(calc.ny, calc.dy)[None, :])
    assert bits[0, 0] == 0 and ((bits & 1) != 0)[(q > 0.035 / lam) & (q < 0.065 / lam)].all()         # fft order: k = 0 at [0, 0]
    assert names.count("tds_fetch") == 2 and names.count("propagate_frame") == 2
    assert [names[i + 1] for i, v in enumerate(names) if v == "propagate_frame"] == ["tds_fetch", "tds_fetch"]
    # shapes and the parts
    nz = calc.nz
    assert res.signals.shape == (3, 1, 2) and res.tds_per_slice.shape == (3, 1, 2, nz)
    assert res.tds.shape == (3, 1, 2) and res.total.shape == (3, 1, 2)
    want = np.zeros((3, 1, 2, nz))
    for p, (call, row) in enumerate(((1, 0), (1, 1), (2, 0))):
        for d in range(2):
            want[p, 0, d] = (100.0 * call + 10.0 * np.arange(nz) + d + row / 10.0) * (calc.nx * calc.ny)     # the units of signals
    assert np.array_equal(res.tds_per_slice, want)
    assert np.array_equal(res.tds, want.sum(axis=-1)) and np.array_equal(res.total, res.signals + res.tds)
    assert np.array_equal(res.image("d1", part="tds") + res.image("d1", part="elastic"), res.image("d1", part="total"))
    assert np.array_equal(res.image("d1"), res.image("d1", part="total"))
    assert res.image("d1", part="tds").max() == want[:, 0, 1].sum(axis=-1).max()
    with pytest.raises(ValueError, match="part must be"):
        res.image("d1", part="thermal")


def test_thickness_axis_is_the_cumulative_sum_at_the_entries(source, monkeypatch):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", TdsEngine)
    calc = _calc(tds=True, detectors=dets(1), thickness=[0, 2])
    _setup(calc, source)
    assert calc.nz == 3
    res = calc.run_detectors()
    assert list(res.layer) == [0, 2]
    per = res.tds_per_slice
    assert per.shape == (3, 1, 1, 3) and res.signals.shape == (3, 1, 1, 2)
    assert res.tds.shape == (3, 1, 1, 2) and res.total.shape == (3, 1, 1, 2)
    assert np.array_equal(res.tds[..., 0], per[..., 0]) and np.array_equal(res.tds[..., 1], per.sum(axis=-1))
    first, last = res.at(0), res.at(-1)
    assert first.tds_per_slice.shape == (3, 1, 1, 1) and np.array_equal(first.tds, res.tds[..., 0])
    assert np.array_equal(last.tds, res.tds[..., 1]) and np.array_equal(last.total, res.total[..., 1])
    assert np.array_equal(res.image("d0", layer=0, part="tds"), first.image("d0", part="tds"))


def test_a_run_without_tds_has_no_tds_and_records_todays_calls(source, monkeypatch):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", TdsEngine)
    seqs = []
    for kw in ({}, dict(tds=False)):
        calc = _calc(detectors=dets(1), probe_batch=2, **kw)
        _setup(calc, source)
        res = calc.run_detectors()
        seqs.append(format_calls(calc._engine.calls, PP))
        assert res.tds_per_slice is None
        with pytest.raises(ValueError, match="no TDS signal"):
            res.tds
        with pytest.raises(ValueError, match="needs a run with"):
            res.image("d0", part="total")
        assert np.array_equal(res.image("d0"), res.image("d0", part="elastic"))
    assert seqs[0] == seqs[1] == [
        "set_kirkland(f8(103,3,4))", "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_absorption(f8(103,), True)",
        "set_detectors(u2(1920,), (intensity), f4(48,), f4(40,))", "build_potential(f8(12,3), i4(12,), 2)",
        "set_probes(30, xy[0,1])", "propagate_frame(0)", "detect(0, 1, B=2)",
        "set_probes(30, xy[2,2])", "propagate_frame(0)", "detect(0, 1, B=1)"]


def test_probe_batch_fit_counts_the_weight_stack(source, monkeypatch):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", TdsEngine)
    got = []
    for tds in (False, True):
        calc = _calc(detectors=dets(4), tds=tds)
        _setup(calc, source)
        # free memory such that the run without TDS just keeps 256 probes: the four weight stacks must cost some of them
        calc.n_probes = 256
        npix = calc.nx * calc.ny
        free = (256 * (32.0 * npix + 8.0 * calc._stored_shape()[2]) + calc._stack_bytes() * calc.nz * npix + calc._phase_table_bytes(1) + 1e9) / 0.9 + 1.0
        got.append(calc._fit_probe_batch(free, 256, 1))
    assert got[0] == 256 and got[1] < 256


# ---- the C ABI ---------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from pyslice_amd import build_native, _native
    build_native.build()
    lib = _native.load()
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    for name, n_args in (("msl_set_tds", 3), ("msl_tds_fetch", 3), ("msl_tds_reduce", 5)):
        m = re.search(r"\bint\s+" + name + r"\(([^)]*)\);", hdr)
        assert m and m.group(1).startswith("msl_handle* h,"), name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _native.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name
    for name, value in (("FORMFACTOR_TDS", 15), ("TDS_WEIGHT", 16)):
        assert re.search(r"\bMSL_BUF_" + name + r" = " + str(value) + r"\b", hdr), name
        assert getattr(_native, "BUF_" + name) == value
    for name in ("set_tds", "tds_fetch", "tds_reduce", "form_factors_tds", "tds_weight"):
        assert callable(getattr(_native.Engine, name))
    import pyslice_amd as ps
    from pyslice_amd import tds
    assert ps.tds_tables is tds.tds_tables and ps.tds_weight is tds.tds_weight and ps.tds_signal is tds.tds_signal
