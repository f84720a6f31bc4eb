"""Absorptive potential, host side: the NumPy definition (pyslice_amd/absorptive.py) against the exact thermal mean of one atom's
transmission, the input type, the calculator's refusals and calls (RecordingEngine: no device), and the C ABI's bindings."""
import os
import re

import numpy as np
import pytest

from oracle import multislice_oracle as orc
from pyslice_amd import absorptive
from pyslice_amd.absorptive import AbsorptivePotential, absorptive_tables, absorptive_transmission, mean_transmission_exact
from pyslice_amd.thermal import FrozenPhonons, sigma_from_B
from recording_engine import RecordingEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV = 100e3
NX, NY, DX, DY, U = 48, 40, 0.1, 0.09, 0.08           # the single-atom case of DESIGN.md section 4.22


def _q2(nx=NX, ny=NY, dx=DX, dy=DY):
    return np.fft.fftfreq(nx, dx)[:, None] ** 2 + np.fft.fftfreq(ny, dy)[None, :] ** 2


def _f(Z, scale=1.0):
    return scale * orc.form_factor(_q2(), Z)


# ---- the tables --------------------------------------------------------------------------------------------
def test_zero_width_is_no_vibration():
    f = _f(6)
    fD, g = absorptive_tables(f, _q2(), 0.0, DX, DY)
    assert np.array_equal(absorptive.debye_waller(_q2(), 0.0), np.ones((NX, NY)))
    assert fD.tobytes() == f.tobytes()
    assert g.shape == f.shape and not g.any()


@pytest.mark.parametrize("Z", [6, 14, 79])
def test_g_is_real_even_and_positive_at_the_origin(Z):
    fD, g = absorptive_tables(_f(Z), _q2(), U, DX, DY, complex_g=True)
    assert np.abs(g.imag).max() <= 1e-12 * np.abs(g.real).max()
    g = g.real
    assert np.array_equal(g, absorptive_tables(_f(Z), _q2(), U, DX, DY)[1])
    mirror_x, mirror_y = np.roll(g[::-1], 1, axis=0), np.roll(g[:, ::-1], 1, axis=1)
    assert np.abs(g - mirror_x).max() <= 1e-12 * np.abs(g).max() and np.abs(g - mirror_y).max() <= 1e-12 * np.abs(g).max()
    assert g[0, 0] > 0
    assert np.array_equal(fD, _f(Z) * np.exp(-2 * np.pi ** 2 * U ** 2 * _q2()))


def _one_atom_errors(Z, scale):
    """max |t - <t>| of one atom at the origin: the absorptive t, and Debye-Waller damping alone"""
    sig = orc.interaction_sigma(EV)
    f, cell = _f(Z, scale), DX ** 2 * DY ** 2
    fD, g = absorptive_tables(f, _q2(), U, DX, DY)
    Vbar, Om = np.fft.ifft2(fD).real / cell, np.fft.ifft2(g).real / cell
    exact = mean_transmission_exact(f, _q2(), U, DX, DY, sig)
    return (np.abs(absorptive_transmission(Vbar, Om, sig) - exact).max(),
            np.abs(absorptive_transmission(Vbar, 0.0 * Om, sig) - exact).max())


def test_single_atom_is_third_order():
    """carbon, 48 x 40, dx 0.1, dy 0.09, u = 0.08 A, 100 keV: the discrepancy to the exact mean falls by at least 7 per halving of
    the table over three halvings (measured 7.9-8.0: third order), and at full scale it is at least 15 x below that of the
    Debye-Waller damping alone (measured 17)"""
    errs = [_one_atom_errors(6, s) for s in (1.0, 0.5, 0.25, 0.125)]
    print("carbon: absorptive", [f"{e[0]:.3e}" for e in errs], "damping alone", [f"{e[1]:.3e}" for e in errs])
    for a, b in zip(errs, errs[1:]):
        assert a[0] / b[0] >= 7.0
    assert errs[0][1] / errs[0][0] >= 15.0
    assert errs[0][0] < 2e-3


def test_two_species_in_one_slice_are_third_order():
    """carbon at the origin and oxygen (u = 0.09) at pixel (20, 17): the exact mean of independent atoms is the product of the two
    single-atom means; Vbar and Omega add, so t is the product of the two absorptive t -- held to the same third-order behaviour"""
    sig, cell, q2 = orc.interaction_sigma(EV), DX ** 2 * DY ** 2, _q2()
    kx, ky = np.fft.fftfreq(NX, DX)[:, None], np.fft.fftfreq(NY, DY)[None, :]
    shift = np.exp(-2j * np.pi * (kx * 20 * DX + ky * 17 * DY))
    errs = []
    for scale in (1.0, 0.5, 0.25, 0.125):
        Vbar = Om = 0.0
        exact = 1.0
        for Z, u, ph in ((6, U, 1.0), (8, 0.09, shift)):
            f = _f(Z, scale)
            fD, g = absorptive_tables(f, q2, u, DX, DY)
            Vbar = Vbar + np.fft.ifft2(fD * ph).real / cell
            Om = Om + np.fft.ifft2(g * ph).real / cell
            one = mean_transmission_exact(f, q2, u, DX, DY, sig)
            exact = exact * np.fft.ifft2(np.fft.fft2(one) * ph)
        errs.append(np.abs(absorptive_transmission(Vbar, Om, sig) - exact).max())
    print("C + O:", [f"{e:.3e}" for e in errs])
    for a, b in zip(errs, errs[1:]):
        assert a / b >= 7.0


# ---- the input type ----------------------------------------------------------------------------------------
def _structure():
    Z = np.array([14, 8, 8, 14, 38, 8], dtype=np.int32)
    pos = np.array([[0.5, 0.5, 0.5], [1.5, 0.7, 1.0], [2.5, 2.0, 1.5], [3.0, 3.1, 2.0], [1.0, 3.0, 2.5], [2.2, 1.1, 0.8]])
    return Z, pos, np.diag([4.0, 4.0, 3.0])


def test_class_shapes_and_widths():
    Z, pos, box = _structure()
    ap = AbsorptivePotential(Z, pos, box, {14: 0.07, "O": 0.09, 38: 0.05})
    assert ap.n_frames == 1 and ap.n_atoms == 6 and ap.positions.shape == (1, 6, 3) and ap.absorption
    assert ap.u_by_Z.shape == (103,) and ap.u_by_Z[13] == 0.07 and ap.u_by_Z[7] == 0.09 and ap.u_by_Z[37] == 0.05
    assert np.count_nonzero(ap.u_by_Z) == 3
    assert AbsorptivePotential(Z, pos, box, float(sigma_from_B(0.5))).u_by_Z[13] == pytest.approx(np.sqrt(0.5 / (8 * np.pi ** 2)))
    assert np.array_equal(AbsorptivePotential(["Si", "O"], pos[:2], box, 0.1).u_by_Z.nonzero()[0], [7, 13])
    with pytest.raises(ValueError, match=r"box_matrix must be \(3, 3\)"):
        AbsorptivePotential(Z, pos, box[:2], 0.1)
    with pytest.raises(ValueError, match=r"positions must be \(atoms, 3\)"):
        AbsorptivePotential(Z, pos[:, :2], box, 0.1)
    with pytest.raises(ValueError, match="Atom count mismatch"):
        AbsorptivePotential(Z[:5], pos, box, 0.1)
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite and >= 0"):
            AbsorptivePotential(Z, pos, box, bad)
    with pytest.raises(ValueError, match="38"):
        AbsorptivePotential(Z, pos, box, {14: 0.07, 8: 0.09})


def test_two_widths_inside_one_element_are_refused_by_name():
    Z, pos, box = _structure()
    with pytest.raises(ValueError, match=r"element O \(Z = 8\) has 2 different widths"):
        AbsorptivePotential(Z, pos, box, np.array([0.07, 0.09, 0.09, 0.07, 0.05, 0.1]))


def test_frozen_phonons_round_trip_and_from_trajectory():
    Z, pos, box = _structure()
    fp = FrozenPhonons(Z, pos, box, {14: 0.07, 8: 0.09, 38: 0.05}, 7, seed=3, timestep=0.5)
    ap = fp.absorptive()
    assert isinstance(ap, AbsorptivePotential) and ap.absorption and not fp.absorptive(absorption=False).absorption
    assert np.array_equal(ap.base_positions, fp.positions) and np.array_equal(ap.sigma, fp.sigma) and ap.timestep == 0.5
    back = ap.frozen_phonons(7, seed=3)
    assert np.array_equal(back.configuration(2), fp.configuration(2))
    tr = fp.to_trajectory()
    ap2 = AbsorptivePotential.from_trajectory(tr, {14: 0.07, 8: 0.09, 38: 0.05}, frame=3)
    assert np.array_equal(ap2.base_positions, tr.positions[3]) and np.array_equal(ap2.u_by_Z, ap.u_by_Z)
    with pytest.raises(ValueError, match="frame 7 outside"):
        AbsorptivePotential.from_trajectory(tr, 0.1, frame=7)
    import pyslice_amd as ps
    assert ps.AbsorptivePotential is AbsorptivePotential and ps.absorptive_tables is absorptive_tables
    assert [len(v) for v in ps.gridFromTrajectory(ap)[:3]] == [len(v) for v in ps.gridFromTrajectory(tr)[:3]]


# ---- the calculator ----------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (4.8, 0.4)]


@pytest.fixture(scope="module")
def source():
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 4, 1, ny=80, density=0.05, seed=4, species=(14, 8))
    return AbsorptivePotential.from_trajectory(tr, {14: 0.078, 8: 0.09})


def _calc(**kw):
    import pyslice_amd as ps
    return ps.MultisliceCalculator(device=0, progress=False, **kw)


def test_refusals_name_the_absorptive_potential(source, monkeypatch, tmp_path):
    from pyslice_amd import _native, distributed
    from pyslice_amd.spectroscopy import Spectroscopy
    from pyslice_amd.stem_data import Detector

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the refusal")
    monkeypatch.setattr(_native, "Engine", no_engine)
    monkeypatch.chdir(tmp_path)
    spec = Spectroscopy(detectors=[Detector("adf", inner=40.0, outer=120.0)])
    for kw in (dict(cache=True), dict(stream_tile=2), dict(spectroscopy=spec)):
        with pytest.raises(NotImplementedError, match=r"absorptive potential: .* is not built"):
            _calc(**kw).setup(source, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r"absorptive potential: .* is not built"):
        _calc().setup(source, aperture=30.0, voltage_eV=EV, probe_positions=PP)


class AbsorptionRecorder(RecordingEngine):
    """RecordingEngine with the new engine method spelled out: a calculator that stops calling it fails with an AttributeError-free,
    readable assertion below"""

    def set_absorption(self, u_by_Z=None, absorb=True):
        self.calls.append(("set_absorption", (None if u_by_Z is None else np.array(u_by_Z), absorb), {}))


@pytest.mark.parametrize("run, kw", [("run", ""), ("run_diffraction", "diffraction"), ("run_detectors", "detectors")])
@pytest.mark.parametrize("absorption", [True, False])
def test_engine_gets_set_absorption_before_the_first_build(source, monkeypatch, run, kw, absorption):
    from pyslice_amd import _native
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.stem_data import Detector
    kw = {"diffraction": dict(diffraction=Diffraction(bin=(2, 2))),
          "detectors": dict(detectors=[Detector("bf", inner=0.0, outer=10.0)])}.get(kw, {})
    monkeypatch.setattr(_native, "Engine", AbsorptionRecorder)
    src = source if absorption else AbsorptivePotential(source.atom_types, source.base_positions, source.box_matrix,
                                                        {14: 0.078, 8: 0.09}, absorption=False)
    calc = _calc(**kw)
    calc.setup(src, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    getattr(calc, run)()
    names = [c[0] for c in calc._engine.calls]
    assert names.count("set_absorption") == 1 and "set_structure" not in names
    assert "build_thermal" not in names and "build_modes" not in names
    builds = [i for i, n in enumerate(names) if n in ("build_potential", "build_potentials")]
    assert len(builds) == 1 and names.index("set_absorption") < builds[0]
    u, absorb = calc._engine.calls[names.index("set_absorption")][1]
    assert np.array_equal(u, src.u_by_Z) and absorb is absorption
    pos, Z = calc._engine.calls[builds[0]][1][:2]
    assert np.array_equal(np.asarray(pos).reshape(-1, 3), src.base_positions) and np.array_equal(Z, np.asarray(src.atom_types))


def test_a_trajectory_run_never_sets_absorption(source, monkeypatch):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", AbsorptionRecorder)
    calc = _calc()
    calc.setup(source.frozen_phonons(1).to_trajectory(), aperture=30.0, voltage_eV=EV, probe_positions=PP)
    calc.run()
    assert "set_absorption" not in [c[0] for c in calc._engine.calls]


# ---- the C ABI ---------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from pyslice_amd import build_native, _native
    build_native.build()
    lib = _native.load()
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"#define MSL_ABI_VERSION 3\b", hdr) and lib.msl_abi_version() == 3
    m = re.search(r"\bint\s+msl_set_absorption\(([^)]*)\);", hdr)
    assert m and m.group(1).startswith("msl_handle* h,")
    n_args = len(m.group(1).split(","))
    assert "msl_set_absorption" in _native.EXPORTS and hasattr(lib, "msl_set_absorption")
    assert len(lib.msl_set_absorption.argtypes) == n_args == 3
    for name, value in (("FORMFACTOR_ABS", 13), ("ABSORPTION", 14)):
        assert re.search(r"\bMSL_BUF_" + name + r" = " + str(value) + r"\b", hdr), name
        assert getattr(_native, "BUF_" + name) == value
    for name in ("set_absorption", "form_factors_abs", "absorption"):
        assert callable(getattr(_native.Engine, name))
    assert lib.msl_set_absorption(None, None, 0) == _native.MSL_ERR_INVALID
