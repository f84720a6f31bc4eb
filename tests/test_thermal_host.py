"""Frozen phonons on the host: the generator's definition (Philox-4x32-10 known answers, uniforms, Box-Muller moments, the
Debye-Waller factor), the FrozenPhonons input type, the three entry points in the header / binding / library, and the calls the
calculator makes for a FrozenPhonons in place of a Trajectory (RecordingEngine: no device)."""
import math
import os
import re

import numpy as np
import pytest

from pyslice_amd import thermal
from pyslice_amd.thermal import FrozenPhonons
from recording_engine import RecordingEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV = 100e3


# ---- Philox ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    """the Random123 known-answer vectors of philox4x32_10"""
    got = thermal.philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_philox_is_elementwise_over_leading_axes():
    ctr = np.arange(24, dtype=np.uint32).reshape(2, 3, 4)
    out = thermal.philox4x32_10(ctr, (7, 9))
    assert out.shape == (2, 3, 4)
    assert np.array_equal(out[1, 2], thermal.philox4x32_10(ctr[1, 2], (7, 9)))


# ---- uniforms and normals ----------------------------------------------------------------------------------
def test_uniforms_are_strictly_inside_the_unit_interval():
    u = thermal.uniforms(np.array([0, 0xffffffff], dtype=np.uint32))
    assert u.dtype == np.float64
    assert 0.0 < u[0] == 2.0 ** -33 and u[1] == 1.0 - 2.0 ** -33 < 1.0
    bound = math.sqrt(2 * 33 * math.log(2))
    r = math.sqrt(-2.0 * math.log(u[0]))                        # the largest radius there is: the bound itself, to rounding
    assert r == pytest.approx(bound, rel=4e-16) and r < 6.77 and bound < 6.77


@pytest.fixture(scope="module")
def g0():
    return thermal.normals(1, 0, 100000)


def test_normals_are_finite_and_bounded(g0):
    assert g0.shape == (100000, 3) and g0.dtype == np.float64
    assert np.isfinite(g0).all()
    assert np.abs(g0).max() <= math.sqrt(2 * 33 * math.log(2)) * (1 + 4e-16) < 6.77


def test_moments(g0):
    """five-sigma bounds of the estimators (N = 3e5 values, fixed seed): mean, variance, the correlation between components and
    between two configurations of the same atoms"""
    N = g0.size
    assert N == 300000
    mean, var = g0.mean(), g0.var()
    print(f"mean {mean:.3e} (bound {5 / math.sqrt(N):.3e}), var - 1 {var - 1:.3e} (bound {5 * math.sqrt(2 / N):.3e})")
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / N)
    bound = 5 / math.sqrt(N / 3)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        c = np.corrcoef(g0[:, a], g0[:, b])[0, 1]
        print(f"corr(g{a}, g{b}) = {c:.3e} (bound {bound:.3e})")
        assert abs(c) <= bound
    g1 = thermal.normals(1, 1, 100000)
    for a in range(3):
        c = np.corrcoef(g0[:, a], g1[:, a])[0, 1]
        print(f"corr(config 0, config 1) of g{a} = {c:.3e}")
        assert abs(c) <= bound


def test_debye_waller_factor():
    """<exp(-2 pi i k u_x)> = exp(-2 pi^2 sigma^2 k^2) = e^-1/2 at k = 1 / (2 pi sigma): 4096 configurations of one atom, standard
    error <= 1/64, bound five times that"""
    sigma = 0.1
    k = 1.0 / (2.0 * math.pi * sigma)
    fp = FrozenPhonons([14], np.zeros((1, 3)), np.diag([5.0, 5.0, 5.0]), sigma, 4096, seed=0)
    ux = np.array([fp.configuration(c)[0, 0] for c in range(4096)])
    got = np.exp(-2j * math.pi * k * ux).mean()
    print(f"<exp(-2 pi i k u)> = {got:.4f}, e^-1/2 = {math.exp(-0.5):.4f}")
    assert abs(got - math.exp(-0.5)) <= 0.08


def test_counter_layout_uses_all_64_bits_of_config_and_seed():
    n = 16
    assert not np.array_equal(thermal.normals(3, 2 ** 32 + 5, n), thermal.normals(3, 5, n))
    assert not np.array_equal(thermal.normals(2 ** 32 + 3, 5, n), thermal.normals(3, 5, n))
    # the definition, spelt out for one atom
    i, c, seed = 11, 2 ** 32 + 5, 2 ** 32 + 3
    x = thermal.philox4x32_10(np.array([i, c & 0xffffffff, c >> 32, 0], dtype=np.uint32), (seed & 0xffffffff, seed >> 32))
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3])]
    assert np.allclose(thermal.normals(seed, c, n)[i], want, rtol=0, atol=1e-14)
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError):
            thermal.normals(bad, 0, 4)
        with pytest.raises(ValueError):
            thermal.normals(0, bad, 4)


def test_sigma_from_B():
    assert thermal.sigma_from_B(8 * math.pi ** 2 * 0.01) == pytest.approx(0.1, rel=1e-15)
    assert np.allclose(thermal.sigma_from_B([0.0, 0.5]), [0.0, math.sqrt(0.5 / (8 * math.pi ** 2))])


# ---- the input type ----------------------------------------------------------------------------------------
def _structure(n=30, seed=5):
    rng = np.random.default_rng(seed)
    Z = np.array([14, 8, 38] * (n // 3) + [14] * (n % 3))
    box = np.diag([9.55, 7.95, 2.75])
    return Z, rng.random((n, 3)) * np.diag(box), box


def test_zero_width_atoms_are_bit_identical():
    Z, pos, box = _structure()
    sig = np.where(np.arange(len(Z)) % 4 == 0, 0.0, 0.08)
    fp = FrozenPhonons(Z, pos, box, sig, 3, seed=9)
    for k in range(3):
        c = fp.configuration(k)
        assert np.array_equal(c[sig == 0].view(np.uint64), pos[sig == 0].view(np.uint64))
        assert (c[sig > 0] != pos[sig > 0]).all()
    assert np.array_equal(thermal.displaced(pos, sig, 9, 2), fp.configuration(2))


def test_width_forms_agree():
    Z, pos, box = _structure()
    by_Z = {14: 0.07, 8: 0.09, 38: 0.05}
    per_atom = np.array([by_Z[z] for z in Z.tolist()])
    a = FrozenPhonons(Z, pos, box, per_atom, 2, seed=1)
    b = FrozenPhonons(Z, pos, box, by_Z, 2, seed=1)
    c = FrozenPhonons(Z, pos, box, {"Si": 0.07, "O": 0.09, "Sr": 0.05}, 2, seed=1)
    assert np.array_equal(a.sigma, b.sigma) and np.array_equal(a.sigma, c.sigma)
    assert np.array_equal(a.configuration(1), b.configuration(1)) and np.array_equal(a.configuration(1), c.configuration(1))
    s = FrozenPhonons(Z, pos, box, 0.07, 2, seed=1)
    u = FrozenPhonons(Z, pos, box, np.full(len(Z), 0.07), 2, seed=1)
    assert np.array_equal(s.configuration(1), u.configuration(1))


def test_width_refusals():
    Z, pos, box = _structure()
    with pytest.raises(ValueError, match="38"):
        FrozenPhonons(Z, pos, box, {14: 0.07, 8: 0.09}, 2)
    for bad in (-0.01, float("nan"), float("inf"), {14: 0.07, 8: -0.09, 38: 0.05}, np.full(len(Z), np.nan), np.full(len(Z) - 1, 0.1)):
        with pytest.raises(ValueError):
            FrozenPhonons(Z, pos, box, bad, 2)


def test_shape_refusals_use_the_messages_of_trajectory():
    Z, pos, box = _structure()
    with pytest.raises(ValueError, match=r"box_matrix must be \(3, 3\)"):
        FrozenPhonons(Z, pos, box[:2], 0.1, 2)
    with pytest.raises(ValueError, match="atom_types must be 1D"):
        FrozenPhonons(Z[None], pos, box, 0.1, 2)
    with pytest.raises(ValueError, match="Atom count mismatch"):
        FrozenPhonons(Z[:-1], pos, box, 0.1, 2)
    with pytest.raises(ValueError, match="positions must be"):
        FrozenPhonons(Z, pos[None], box, 0.1, 2)
    with pytest.raises(ValueError, match="n_configs"):
        FrozenPhonons(Z, pos, box, 0.1, 0)


def test_to_trajectory_is_the_definition_and_validates():
    import pyslice_amd as ps
    Z, pos, box = _structure()
    fp = FrozenPhonons(Z, pos, box, 0.06, 4, seed=2 ** 40 + 1, timestep=0.5)
    assert (fp.n_frames, fp.n_configs, fp.n_atoms, fp.timestep) == (4, 4, 30, 0.5)
    assert np.array_equal(fp.box_tilts, [0.0, 0.0, 0.0])
    tr = fp.to_trajectory()
    assert isinstance(tr, ps.Trajectory) and tr.positions.shape == (4, 30, 3) and tr.timestep == 0.5
    for k in range(4):
        assert np.array_equal(tr.positions[k], fp.configuration(k))
    ps.Trajectory(tr.atom_types, tr.positions, tr.velocities, tr.box_matrix, tr.timestep)        # validates
    assert np.array_equal(fp.to_trajectory([3, 1]).positions, tr.positions[[3, 1]])
    back = FrozenPhonons.from_trajectory(tr, 0.06, 4, seed=2 ** 40 + 1, frame=2)
    assert np.array_equal(back.positions, tr.positions[2]) and back.timestep == 0.5
    assert ps.FrozenPhonons is FrozenPhonons
    # the grid helpers take it as they take a Trajectory
    assert [len(v) for v in ps.gridFromTrajectory(fp)[:3]] == [len(v) for v in ps.gridFromTrajectory(tr)[:3]]


# ---- the C ABI ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pyslice_amd import build_native, _native
    build_native.build()
    return _native.load()


def test_entry_points_in_the_header_binding_and_library(lib):
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"#define MSL_ABI_VERSION 3\b", hdr) and lib.msl_abi_version() == 3
    for name in ("msl_set_structure", "msl_build_thermal", "msl_thermal_positions"):
        assert re.search(r"\bint\s+" + name + r"\(msl_handle\* h,", hdr), name
        assert name in _native.EXPORTS and hasattr(lib, name), name
    for name in ("set_structure", "build_thermal", "thermal_positions"):
        assert callable(getattr(_native.Engine, name))
    assert lib.msl_build_thermal(None, 0, 0, 1) == _native.MSL_ERR_INVALID
    assert lib.msl_thermal_positions(None, 0, 0, None) == _native.MSL_ERR_INVALID
    assert lib.msl_set_structure(None, None, None, None, 0, 0, 1, 2) == _native.MSL_ERR_INVALID


# ---- the calculator ----------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (4.8, 0.4), (0.0, 0.0), (2.5, 2.5)]
SEED = 2 ** 33 + 17


@pytest.fixture(scope="module")
def phonons():
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, 1, ny=80, density=0.05, seed=4, species=(79, 6))
    return FrozenPhonons.from_trajectory(tr, {79: 0.05, "C": 0.09}, 5, seed=SEED)


def _calc(**kw):
    import pyslice_amd as ps
    return ps.MultisliceCalculator(device=0, progress=False, **kw)


def _recorded(monkeypatch, source, run, **kw):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    calc = _calc(**kw)
    calc.setup(source, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    getattr(calc, run)()
    return calc._engine.calls


def _modes():
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.stem_data import Detector
    return [("run", {}),
            ("run_detectors", dict(detectors=[Detector("adf", inner=40.0, outer=120.0)], probe_batch=2)),
            ("run_diffraction", dict(diffraction=Diffraction(bin=(2, 2), split=True), probe_batch=2))]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_calculator_builds_by_index(phonons, monkeypatch, mode):
    """5 configurations at frame_batch = 2 (two probe batches in the probe-batch modes): one set_structure, and build_thermal with
    exactly the (s0, n) sequence build_potentials gets for the 5-frame Trajectory of the same configurations; everything else the
    engine is asked to do is the same, call for call"""
    run, kw = _modes()[mode]
    tr = phonons.to_trajectory()
    got = _recorded(monkeypatch, phonons, run, frame_batch=2, **kw)
    ref = _recorded(monkeypatch, tr, run, frame_batch=2, **kw)
    structure = [c for c in got if c[0] == "set_structure"]
    assert len(structure) == 1
    pos, Z, sigma, axis = structure[0][1]
    assert np.array_equal(pos, phonons.positions) and np.array_equal(sigma, phonons.sigma) and axis == 2
    assert np.array_equal(Z, tr.atom_types) and Z.dtype == np.int32
    assert not [c for c in got if c[0] in ("build_potential", "build_potentials")]
    thermal_calls = [c[1] for c in got if c[0] == "build_thermal"]
    assert all(a[0] == SEED for a in thermal_calls)

    def first_frame(block):
        hits = [s for s in range(5) if np.array_equal(tr.positions[s:s + len(block)], block)]
        assert len(hits) == 1
        return hits[0]
    want = [(first_frame(c[1][0]), len(c[1][0])) for c in ref if c[0] == "build_potentials"]
    assert len(want) >= 3 and [(a[1], a[2]) for a in thermal_calls] == want
    if run == "run_diffraction":
        assert want == 2 * [(0, 2), (2, 2), (4, 1)]             # once per probe batch: a regeneration by index
    # the rest of the two recordings, in order
    rest = lambda calls: [c[0] for c in calls if c[0] not in ("set_structure", "build_thermal", "build_potentials")]
    where = lambda calls, name: [i for i, c in enumerate(calls) if c[0] == name]
    assert rest(got) == rest(ref)
    assert [i - 1 for i in where(got, "build_thermal")] == where(ref, "build_potentials")       # (set_structure is one call earlier)


def test_prism_loop_builds_by_index_at_frame_batch_one(phonons, monkeypatch):
    from pyslice_amd.prism import Prism
    from pyslice_amd.stem_data import Detector
    kw = dict(detectors=[Detector("adf", inner=40.0, outer=120.0)], probe_batch=2, prism=Prism(1))
    got = _recorded(monkeypatch, phonons, "run_detectors", **kw)
    assert [c[1] for c in got if c[0] == "build_thermal"] == [(SEED, s, 1) for s in range(5)]
    assert len([c for c in got if c[0] == "set_structure"]) == 1
    assert not [c for c in got if c[0] in ("build_potential", "build_potentials")]
    assert [c[0] for c in got if c[0] in ("build_thermal", "smatrix_build")] == 5 * ["build_thermal", "smatrix_build"]
    got = _recorded(monkeypatch, phonons, "run", prism=Prism(1))
    assert [c[1] for c in got if c[0] == "build_thermal"] == [(SEED, s, 1) for s in range(5)]
    assert not [c for c in got if c[0] in ("build_potential", "build_potentials")]


def test_a_trajectory_run_is_unchanged(phonons, monkeypatch):
    """a Trajectory never reaches the new calls, at either frame batch"""
    tr = phonons.to_trajectory()
    for fb, name in ((1, "build_potential"), (2, "build_potentials")):
        calls = _recorded(monkeypatch, tr, "run", frame_batch=fb)
        assert not [c for c in calls if c[0] in ("set_structure", "build_thermal")]
        assert len([c for c in calls if c[0] == name]) == (5 if fb == 1 else 3)


def test_refusals_name_frozen_phonons(phonons, monkeypatch, tmp_path):
    from pyslice_amd import _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(_native, "Engine", no_engine)
    monkeypatch.chdir(tmp_path)
    for kw in (dict(cache=True), dict(stream_tile=2)):
        with pytest.raises(NotImplementedError, match=r"frozen phonons: .* is not built"):
            _calc(**kw).setup(phonons, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    assert not os.path.exists(tmp_path / "psi_data")           # refused before the cache directory is made
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r"frozen phonons: .* is not built"):
        _calc().setup(phonons, aperture=30.0, voltage_eV=EV, probe_positions=PP)
