"""Gradients with respect to scan positions and probe aberrations, host side (no GPU): the float64
definition (adjoint.probe_spectrum / probe_parameter_gradient) against the reference's probe goldens and against Richardson-extrapolated
central differences of adjoint.total_loss; the sensitivity of the device bound to faults built into the chain, on the device test's own
inputs; a complex64 model of the chain; the calculator on a recording engine; the ABI."""
import dataclasses
import os
import re

import numpy as np
import pytest

import gradient_cases as gc
import probe_gradient_cases as pc
from conftest import rel_l2
from recording_engine import RecordingEngine
from pyslice_amd.aberrations import TERMS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AX = (-2, -1)


# ---- 1. the spectrum against the goldens ----
@pytest.mark.parametrize("tag", ["64", "96x80"])
@pytest.mark.parametrize("dz", [100.0, 1000.0])
def test_spectrum_reproduces_the_defocus_goldens(golden, tag, dz):
    from pyslice_amd import Aberrations
    from pyslice_amd.adjoint import probe_spectrum
    from pyslice_amd.multislice import wavelength
    g = golden("g10_defocus")
    xs, ys = g[f"xs_{tag}"], g[f"ys_{tag}"]
    Phi = probe_spectrum(len(xs), len(ys), xs[1] - xs[0], ys[1] - ys[0], wavelength(float(g["eV"])), float(g["mrad"]), [(0.0, 0.0)],
                         Aberrations(defocus=dz))
    assert rel_l2(np.fft.ifft2(Phi[0]), g[f"defocus_{tag}_{dz:g}"]) < 1e-12


@pytest.mark.parametrize("name", ["g5_probes", "g5_probes_96x80"])
def test_spectrum_reproduces_the_probe_goldens(golden, name):
    from pyslice_amd.adjoint import probe_spectrum
    from pyslice_amd.multislice import wavelength
    g = golden(name)
    xs, ys = g["xs"], g["ys"]
    eV = float(golden("g5_probes")["eV"])
    Phi = probe_spectrum(len(xs), len(ys), xs[1] - xs[0], ys[1] - ys[0], wavelength(eV), 30.0, g["positions"])
    assert rel_l2(np.fft.ifft2(Phi, axes=AX), g["batch_30"]) < 1e-12


# ---- 2. the definition against finite differences ----
def richardson(f, h):
    """the central difference of f at 0 with steps h, h / 2 and h / 4, extrapolated twice: O(h^6)"""
    d1, d2, d4 = ((f(s) - f(-s)) / (2 * s) for s in (h, h / 2, h / 4))
    e1, e2 = (4.0 * d2 - d1) / 3.0, (4.0 * d4 - d2) / 3.0
    return (16.0 * e2 - e1) / 15.0


FD_GRIDS = [(24, 20, 3), (25, 21, 2)]
POLAR_TERMS = [("C12", "phi12", 10.0), ("C21", "phi21", 100.0), ("C32", "phi32", 1e4)]      # (C, phi, the size of a step in C)
# the scale of a step in every Cartesian coefficient: what 10 A (n = 1), 100 A, 1e4 A, 1e5 A, 1e6 A (n = 5) of C_nm make
CART_SCALE = np.array([10.0, 10.0, 100.0, 100.0, 1e4, 1e4, 1e4, 1e5, 1e5, 1e5, 1e6, 1e6, 1e6, 1e6]) / (np.array([2, 2, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6, 6]) * 0.037)


@pytest.mark.parametrize("grid", FD_GRIDS)
@pytest.mark.parametrize("loss", gc.LOSSES)
@pytest.mark.parametrize("aberrated", [True, False], ids=["aberrated", "zero"])
def test_definition_against_finite_differences(grid, loss, aberrated):
    from pyslice_amd import Aberrations
    from pyslice_amd import adjoint as adj
    c = gc.case(*grid)
    nx, ny = grid[:2]
    geom = pc.run_geometry(grid)
    lam = geom[4]
    P = 2 if grid[2] == 2 else 3
    xy = np.asarray(pc.PP[:P], dtype=np.float64)
    D = c["D"][:P]
    ab = Aberrations(defocus=80.0, astigmatism=30.0, astigmatism_angle=0.4, coma=500.0, coma_angle=1.1, Cs=2.0e5, C32=3e4, phi32=-0.7) \
        if aberrated else Aberrations(C12=0.0)
    cart0 = adj.aberration_cartesian(ab, lam)
    kw = dict(loss=loss, epsilon=gc.epsilon_of(c, loss))
    L = lambda xy_, cart_: adj.probe_loss(*geom, xy_, c["V"], D, c["sigma"], c["prop"], cartesian=cart_, **kw)
    probes = np.fft.ifft2(adj.probe_spectrum(*geom, xy, cartesian=cart0), axes=AX)
    g0 = adj.potential_gradient(probes, c["V"], D, c["sigma"], c["prop"], **kw)[2]
    pos, cart, per = adj.probe_parameter_gradient(g0, *geom, xy, cartesian=cart0)
    assert np.allclose(per.sum(axis=0), cart, rtol=1e-13, atol=0) and not cart[[0, 4, 10], 1].any()
    # positions of 2 probes
    fd_pos = np.zeros((2, 2))
    for p in range(2):
        for a in range(2):
            e = np.zeros_like(xy)
            e[p, a] = 1.0
            fd_pos[p, a] = richardson(lambda s: L(xy + s * e, cart0), 2e-3)
    worst = np.abs(fd_pos - pos[:2]).max() / np.abs(pos).max()
    print(f"{grid} {loss}: positions fd / definition {worst:.2e}")
    assert worst < 1e-6
    # the 25 Cartesian coefficients, in steps of their own scale: compared in those units
    fd_cart = np.zeros((14, 2))
    for j in range(14):
        for b in range(2):
            if b and j in (0, 4, 10):
                continue
            e = np.zeros((14, 2))
            e[j, b] = CART_SCALE[j]
            fd_cart[j, b] = richardson(lambda s: L(xy, cart0 + s * e), 2e-3)
    scaled = cart * CART_SCALE[:, None]
    worst = np.abs(fd_cart - scaled).max() / np.abs(scaled).max()
    print(f"{grid} {loss}: Cartesian fd / definition {worst:.2e}")
    assert worst < 1e-6
    # C_nm and phi_nm of three terms with m != 0 (at the zero set phi has no effect: its derivative is zero)
    dC, dphi = adj.aberration_polar_gradient(cart, ab, lam)
    base = {f.name: getattr(ab, f.name) for f in dataclasses.fields(ab)}
    names = [t[0] for t in TERMS]
    fd_pol, want_pol = [], []
    for cname, pname, step in POLAR_TERMS:                  # in units of the step: Angstrom-sized and radian-sized derivatives side by side
        j = names.index(cname)
        for field, h, want in ((cname, 2e-3 * step, dC[j]), (pname, 2e-3, dphi[j])):
            f = lambda s: L(xy, adj.aberration_cartesian(Aberrations(**{**base, field: base[field] + s}), lam))
            fd_pol.append(richardson(f, h) * h)
            want_pol.append(want * h)
    fd_pol, want_pol = np.array(fd_pol), np.array(want_pol)
    worst = np.abs(fd_pol - want_pol).max() / np.abs(want_pol).max()
    print(f"{grid} {loss}: polar fd / definition {worst:.2e}")
    assert worst < 1e-6
    if not aberrated:
        assert not dphi.any()


# ---- 3. faults against the device bound, on the device test's inputs ----
CHAIN_FAULTS = [f for f in pc.FAULTS if f not in ("no_n_plus_1", "no_m")]


def test_aperture_sizes():
    for case in pc.CHAIN_CASES[1:]:
        assert pc.aperture_pixels(case) >= 100, case
    last = pc.CHAIN_CASES[-1]
    radius = last.mrad * 1e-3 / pc.wavelength()                      # larger than the grid: the box is all of it, Nyquist lines inside
    assert pc.box_axis(last.nx, 1.0 / (last.nx * pc.DX), radius) == (-6, 12) and pc.box_axis(last.ny, 1.0 / (last.ny * pc.DX), radius) == (-525, 1050)
    assert pc.aperture_pixels(last) > 0.8 * last.nx * last.ny
    first = pc.CHAIN_CASES[0]
    r0 = first.mrad * 1e-3 / pc.wavelength()
    assert pc.box_axis(first.nx, 1.0 / (first.nx * pc.DX), r0)[1] * pc.box_axis(first.ny, 1.0 / (first.ny * pc.DX), r0)[1] < pc.PM_TILE     # less than one tile


@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=lambda c: c.name)
def test_faults_miss_the_device_bound(case):
    """Every fault moves some component by at least 10 bounds on every grid where it is a fault at all.  Not detectable, and why:
    le_aperture -- no pixel of any grid lies exactly on the radius, so `<=` and `<` select the same pixels (asserted below: the
    fault is no fault on these inputs); nyquist_sign -- only where an even length has its Nyquist line inside the aperture, 12 x 1050."""
    for aberrated in (True, False):
        want, bound = pc.chain_reference(case, aberrated)
        assert pc.ratio(pc.model(case, aberrated), want, bound) < 1e-3      # (the model is the definition, to rounding)
        for fault in CHAIN_FAULTS:
            got = pc.model(case, aberrated, fault=fault)
            live = bound > 0
            r = float((np.abs(got - want)[live] / bound[live]).max())
            print(f"{case.name} {'aberrated' if aberrated else 'zero'}: fault {fault} / bound {r:.3e}")
            if fault == "le_aperture" or (fault == "nyquist_sign" and case.name != "12x1050"):
                assert r < 1e-3                                      # (no fault on these inputs: the model's own rounding)
            else:
                assert r >= 10.0, (fault, r)
        # the polar chain, at the aberration set (its bound: the Cartesian bound through the same chain in absolute values)
        ab = pc.aberr()
        pw, pb = pc.polar(want, ab), pc.polar_bound(bound, ab)
        for fault in ("no_n_plus_1", "no_m"):
            pg = pc.polar(want, ab, fault=fault)
            live = pb > 0
            r = float((np.abs(pg - pw)[live] / pb[live]).max())
            print(f"{case.name}: fault {fault} / polar bound {r:.3e}")
            assert r >= 10.0, (fault, r)


# ---- 4. the precision model ----
@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=lambda c: c.name)
def test_complex64_model_stays_under_a_third_of_the_bound(case):
    ghat = pc.c64_ghat(case)
    for aberrated in (True, False):
        want, bound = pc.chain_reference(case, aberrated)
        r = pc.ratio(pc.model(case, aberrated, ghat=ghat), want, bound)
        print(f"{case.name} {'aberrated' if aberrated else 'zero'}: complex64 model / bound {r:.3e}")
        assert r <= 1.0 / 3.0


# ---- 5. the calculator on a recording engine ----
class ProbeRecorder(RecordingEngine):
    def __init__(self, nx, ny, nz, *a, **k):
        super().__init__(nx, ny, nz, *a, **k)
        self._shape = (nx, ny, nz)

    def adjoint_add(self, data, B=None, probe=False):
        self.calls.append(("adjoint_add", (data,), dict(B=B, probe=probe)))
        return np.arange(B, dtype=np.float64) + 1.0, None

    def adjoint_download(self):
        self.calls.append(("adjoint_download", (), {}))
        nx, ny, nz = self._shape
        return np.ones((nz, nx, ny))

    def adjoint_probe_params(self, g0=None, B=None):
        self.calls.append(("adjoint_probe_params", (g0,), dict(B=B)))
        return np.arange(B * 30, dtype=np.float64).reshape(B, 30) + 1.0


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    made = []

    def make(*a, **k):
        made.append(ProbeRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(_native, "Engine", make)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    return made


def setup_calc(ps, recorder, aperture=30.0, aberrations=None, **kw):
    calc = ps.MultisliceCalculator(device=0, progress=False, aberrations=aberrations, **kw)
    calc.setup(gc.trajectory(96, 80, 4), aperture=aperture, voltage_eV=gc.EV, probe_positions=gc.PP, sampling=0.1, slice_thickness=1.0)
    return calc, recorder[-1]


TODAY = ["build_potential", "adjoint_reset"] + ["set_probes", "adjoint_add"] * 2 + ["adjoint_download"]
WITH_PARAMS = ["build_potential", "adjoint_reset"] + ["set_probes", "adjoint_add", "adjoint_probe_params"] * 2 + ["adjoint_download"]


def test_calculator_calls_overrides_and_errors(recorder):
    import pyslice_amd as ps
    from pyslice_amd import Aberrations
    from pyslice_amd.multislice import wavelength
    data = np.ones((3, 96, 80))
    lens = Aberrations(defocus=50.0, astigmatism=20.0, astigmatism_angle=0.3)
    calc, eng = setup_calc(ps, recorder, aberrations=lens, gradient=ps.Gradient(probe_positions=True, aberrations=True), probe_batch=2)
    eng.calls.clear()
    res = calc.run_gradient(data)
    assert [c[0] for c in eng.calls] == WITH_PARAMS
    params = [c for c in eng.calls if c[0] == "adjoint_probe_params"]
    assert [c[2]["B"] for c in params] == [2, 1] and all(c[1] == (None,) for c in params)      # the work buffer; a ragged last batch
    rows = np.concatenate([np.arange(60).reshape(2, 30) + 1.0, np.arange(30).reshape(1, 30) + 1.0])
    assert np.array_equal(res.probe_position_gradient, rows[:, :2]) and res.probe_position_gradient.dtype == np.float64
    cart = rows[:, 2:].sum(axis=0).reshape(14, 2)
    assert np.array_equal(res.aberration_gradient_cartesian, cart)
    lam = wavelength(gc.EV)
    assert set(res.aberration_gradient) == {f for f in Aberrations.__dataclass_fields__ if f[0] in "Cp" and f not in ("Cs", "C5")}
    assert res.aberration_gradient["C10"] == pytest.approx(cart[0, 0] / (2 * lam), rel=1e-14)
    assert res.aberration_gradient["C12"] == pytest.approx((np.cos(0.6) * cart[1, 0] + np.sin(0.6) * cart[1, 1]) / (2 * lam), rel=1e-13)
    assert res.aberration_gradient["phi12"] == pytest.approx(2 * 20.0 / (2 * lam) * (-np.sin(0.6) * cart[1, 0] + np.cos(0.6) * cart[1, 1]), rel=1e-13)
    assert res.aberration_gradient["phi21"] == 0.0                   # (C21 = 0: the angle has no effect)
    assert np.array_equal(res.probe_positions, gc.PP)                # stays the scan positions
    # the steps
    xy = np.asarray(gc.PP)
    assert np.array_equal(res.probe_position_step(xy, 0.5), xy - 0.5 * res.probe_position_gradient)
    with pytest.raises(ValueError, match="probe_position_step"):
        res.probe_position_step(xy[:2], 0.5)
    stepped = res.aberration_step(lens, {"C10": 1e-3, "phi12": 1e-6})
    assert stepped.C10 == lens.C10 - 1e-3 * res.aberration_gradient["C10"] and stepped.phi12 == lens.phi12 - 1e-6 * res.aberration_gradient["phi12"]
    assert stepped.C12 == lens.C12 and stepped.C30 == 0.0
    assert res.aberration_step(lens, 1e-3).C30 == -1e-3 * res.aberration_gradient["C30"]
    with pytest.raises(ValueError, match="aberration_step"):
        res.aberration_step(lens, {"C31": 1.0})
    with pytest.raises(ValueError, match="aberration_step"):
        res.aberration_step("lens", 1.0)
    # the overrides: set_aberrations, the caller's positions per batch, and the restoration
    eng.calls.clear()
    moved = xy + 0.1
    other = Aberrations(defocus=70.0)
    res = calc.run_gradient(data, probe_positions=moved, aberrations=other)
    names = [c[0] for c in eng.calls]
    assert names == WITH_PARAMS[:2] + ["set_aberrations"] + WITH_PARAMS[2:-1] + ["set_aberrations", "adjoint_download"]
    sets = [c for c in eng.calls if c[0] == "set_aberrations"]
    assert sets[0][1] == (other,) and sets[1][1] == (lens,)
    sp = [c for c in eng.calls if c[0] == "set_probes"]
    assert np.array_equal(sp[0][1][1], moved[:2]) and np.array_equal(sp[1][1][1], moved[[2, 2]])
    assert np.array_equal(res.probe_positions, moved)
    assert res.aberration_gradient["C10"] == pytest.approx(cart[0, 0] / (2 * lam), rel=1e-14) and res.aberration_gradient["phi12"] == 0.0
    eng.calls.clear()
    calc.run_gradient(data)                                          # ... and the next plain call is today's
    assert [c[0] for c in eng.calls] == WITH_PARAMS
    assert np.array_equal([c for c in eng.calls if c[0] == "set_probes"][0][1][1], xy[:2])

    class Boom(RuntimeError):
        pass

    def failing(*a, **k):
        raise Boom()
    eng.adjoint_add = failing
    eng.calls.clear()
    with pytest.raises(Boom):
        calc.run_gradient(data, aberrations=other)
    assert eng.calls[-1][0] == "set_aberrations" and eng.calls[-1][1] == (lens,)       # restored behind a failure too
    del eng.adjoint_add
    # ValueErrors
    for bad in (moved[:2], np.full((3, 2), np.nan), np.zeros((3, 3)), "xy"):
        with pytest.raises(ValueError, match="probe_positions"):
            calc.run_gradient(data, probe_positions=bad)
    with pytest.raises(ValueError, match="aberrations"):
        calc.run_gradient(data, aberrations={"defocus": 1.0})
    # one flag alone
    calc, eng = setup_calc(ps, recorder, gradient=ps.Gradient(probe_positions=True), probe_batch=2)
    res = calc.run_gradient(data)
    assert res.probe_position_gradient is not None and res.aberration_gradient is None and res.aberration_gradient_cartesian is None
    with pytest.raises(ValueError, match="aberration_step"):
        res.aberration_step(lens, 1.0)
    calc, eng = setup_calc(ps, recorder, gradient=ps.Gradient(aberrations=True), probe_batch=2)
    res = calc.run_gradient(data)
    assert res.probe_position_gradient is None and res.aberration_gradient["C30"] == pytest.approx(cart[4, 0] / (4 * lam), rel=1e-14)
    with pytest.raises(ValueError, match="probe_position_step"):
        res.probe_position_step(xy, 1.0)


def test_without_the_flags_the_calls_are_todays(recorder):
    import pyslice_amd as ps
    data = np.ones((3, 96, 80))
    calc, eng = setup_calc(ps, recorder, gradient=ps.Gradient(), probe_batch=2)
    eng.calls.clear()
    res = calc.run_gradient(data)
    assert [c[0] for c in eng.calls] == TODAY
    assert res.probe_position_gradient is None and res.aberration_gradient is None and res.aberration_gradient_cartesian is None
    assert "probe_positions" not in repr(ps.Gradient()) and "aberrations" not in repr(ps.Gradient())
    assert "probe_positions=True" in repr(ps.Gradient(probe_positions=True)) and "aberrations=True" in repr(ps.Gradient(aberrations=True))
    # the overrides work without the flags too: a refinement of the potential at other positions
    eng.calls.clear()
    calc.run_gradient(data, probe_positions=np.asarray(gc.PP) + 0.1)
    assert [c[0] for c in eng.calls] == TODAY


def test_refusals(recorder):
    import pyslice_amd as ps
    data = np.ones((3, 96, 80))
    calc, eng = setup_calc(ps, recorder, aperture=0.0, gradient=ps.Gradient(probe_positions=True), probe_batch=2)
    with pytest.raises(NotImplementedError, match=r"gradient: .*plane-wave illumination \(aperture=0\) is not built"):
        calc.run_gradient(data)
    calc, eng = setup_calc(ps, recorder, aperture=0.0, gradient=ps.Gradient(), probe_batch=2)
    calc.run_gradient(data)                                          # the plane-wave run of today stays
    from pyslice_amd.coherence import Coherence
    for kw in (dict(coherence=Coherence(focal_spread=20.0)), dict(k_bin=(2, 2)), dict(layers=[1, 3])):
        with pytest.raises(NotImplementedError, match="gradient: .* is not built"):
            ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(aberrations=True), **kw)


# ---- the definition's argument checks and the ABI ----
def test_definition_argument_checks():
    from pyslice_amd import adjoint as adj
    geom = (8, 6, 0.1, 0.1, 0.037, 300.0)
    g0 = np.random.default_rng(0).standard_normal((2, 8, 6)) + 0j
    with pytest.raises(ValueError, match="g0"):
        adj.probe_parameter_gradient(g0, *geom, [(0.1, 0.2)])
    pos, cart, per = adj.probe_parameter_gradient(g0, *geom, [(0.1, 0.2), (0.3, 0.1)])
    assert pos.shape == (2, 2) and cart.shape == (14, 2) and per.shape == (2, 14, 2)
    bp, bc = adj.probe_parameter_bound(g0, *geom, 1.0)
    assert (np.abs(pos) <= bp).all() and (np.abs(per) <= bc).all()   # (tol = 1: Cauchy-Schwarz on the moment itself)


def test_abi():
    from pyslice_amd import _native
    header = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"^int\s+msl_adjoint_probe_params\(msl_handle\* h, const void\* g0_c64_or_null, int32_t B, double\* out\);", header, re.M)
    assert re.search(r"^int\s+msl_adjoint_probe_params_time\(msl_handle\* h, int32_t reps, double\* ms_chain\);", header, re.M)
    for name in ("msl_adjoint_probe_params", "msl_adjoint_probe_params_time"):
        assert name in _native.EXPORTS
    for name in ("adjoint_probe_params", "adjoint_probe_params_time"):
        assert callable(getattr(_native.Engine, name))
    eng = _native.Engine.__new__(_native.Engine)
    eng.nx, eng.ny, eng.n_probes = 8, 6, 2
    with pytest.raises(ValueError, match="g0 must be"):
        eng.adjoint_probe_params(np.zeros((2, 8, 5), dtype=np.complex64))
    with pytest.raises(ValueError, match="g0 must be"):
        eng.adjoint_probe_params(np.zeros((2, 8, 6), dtype=np.complex64), B=1)
