"""Finite projection, host side: the float64 definitions of pyslice_amd/projection.py against the oracle and
direct quadrature, the tail-folding invariant, the z-centroid, convergence in the node count, and the API.  No GPU."""
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = [(1.0, 1.0), (2.0, 1.5)]


@pytest.fixture(scope="module")
def orc():
    from oracle import multislice_oracle
    return multislice_oracle


@pytest.fixture(scope="module")
def pj():
    from pyslice_amd import projection
    return projection


# ---- finite_form_factor -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z", [1, 6, 14, 79, 103])
def test_whole_axis_is_the_projected_form_factor(pj, orc, Z):
    k2 = np.concatenate([[0.0], np.geomspace(1e-4, 400.0, 60)])
    got, want = pj.finite_form_factor(Z, k2, -np.inf, np.inf), orc.form_factor(k2, Z)
    assert np.max(np.abs(got - want) / np.abs(want)) < 1e-14


@pytest.mark.parametrize("Z", [6, 79])
def test_additive_over_adjacent_slabs(pj, Z):
    k2 = np.geomspace(1e-3, 100.0, 30)
    edges = [-np.inf, -1.3, -0.5, -0.01, 0.0, 0.2, 0.7, 3.0, np.inf]
    parts = sum(pj.finite_form_factor(Z, k2, a, b) for a, b in zip(edges[:-1], edges[1:]))
    whole = pj.finite_form_factor(Z, k2, -np.inf, np.inf)
    assert np.max(np.abs(parts - whole) / whole) < 1e-14
    mid = pj.finite_form_factor(Z, k2, -0.5, 0.2) + pj.finite_form_factor(Z, k2, 0.2, 0.7)
    assert np.max(np.abs(mid - pj.finite_form_factor(Z, k2, -0.5, 0.7)) / np.abs(mid)) < 1e-14


@pytest.mark.parametrize("Z,k2,alpha,beta", [(6, 0.0, -0.25, 0.25), (14, 0.5, 0.1, 0.6), (79, 4.0, -0.75, -0.25), (79, 0.04, -0.3, 1.1),
                                             (6, 25.0, 0.0, 0.5)])
def test_against_quadrature_of_the_kz_integral(pj, orc, Z, k2, alpha, beta):
    """F_Z(k; alpha, beta) = int dk_z f(k^2 + k_z^2) int_alpha^beta exp(2 pi i k_z zeta) dzeta
                           = 2 int_0^inf f(k^2 + k_z^2) [sin(2 pi k_z beta) - sin(2 pi k_z alpha)] / (2 pi k_z) dk_z.
    Head [0, 1] by adaptive quadrature of the regular integrand, tail [1, inf) as two Fourier integrals (QAWF).  The bound is the
    sum of the quadrature's own error estimates, plus 4 ulp of the value for where those fall below float64 rounding."""
    from scipy.integrate import quad
    f = lambda kz: float(orc.form_factor(np.array([k2 + kz * kz]), Z)[0])
    head = lambda kz: 2.0 * f(kz) * (beta * np.sinc(2.0 * kz * beta) - alpha * np.sinc(2.0 * kz * alpha))
    total, err = quad(head, 0.0, 1.0, epsabs=1e-13, epsrel=1e-13, limit=200)
    for edge, sign in ((beta, 1.0), (alpha, -1.0)):
        if edge == 0.0:
            continue
        v, e = quad(lambda kz: 2.0 * f(kz) / (2.0 * np.pi * kz), 1.0, np.inf, weight="sin", wvar=2.0 * np.pi * edge, epsabs=1e-12, limit=400)
        total, err = total + sign * v, err + e
    got = float(pj.finite_form_factor(Z, np.array([k2]), alpha, beta)[0])
    assert abs(got - total) <= err + 4 * np.finfo(float).eps * abs(got), (got, total, err)


def test_channel_tables_layout_and_sum(pj, orc):
    nx, ny, dx, dy, dz, R, J = 12, 10, 0.2, 0.25, 0.5, 2, 3
    t = pj.channel_tables([6, 79], nx, ny, dx, dy, dz, R, J)
    M = (2 * R + 1) * J
    assert t.shape == (2 * M, nx, ny)
    k2 = np.fft.fftfreq(nx, dx)[:, None] ** 2 + np.fft.fftfreq(ny, dy)[None, :] ** 2
    for i, Z in enumerate([6, 79]):
        for r in range(J):                                      # the 2 R + 1 channels of a node: m = r - R J + t J
            node = sum(t[i * M + r + tt * J] for tt in range(2 * R + 1))
            assert np.max(np.abs(node - orc.form_factor(k2, Z)) / orc.form_factor(k2, Z)) < 1e-13
    assert np.allclose(t[M + R * J], pj.finite_form_factor(79, k2, 0.0, dz), rtol=1e-15)     # m = 0: the node's own slab


# ---- finite_potential ---------------------------------------------------------------------------------------------------------------

def _grid(nx=16, ny=12, nz=12, d=0.25, dz=0.5):
    return np.arange(nx) * d, np.arange(ny) * d, np.arange(nz) * dz


@pytest.mark.parametrize("R,J,slice_axis", [(1, 1, 2), (2, 4, 2), (3, 2, 2), (2, 3, 0)])
def test_tail_folding_keeps_the_projected_potential(pj, orc, R, J, slice_axis):
    """atoms at least (R + 1) dz inside the stack: the sum over the slices is the infinite projection's"""
    if slice_axis == 2:
        xs, ys, zs = _grid()
    else:
        xs, ys, zs = np.arange(14) * 0.5, np.arange(12) * 0.25, np.arange(5) * 0.5          # slices along x: the slabs are dx thick
    coords = [xs, ys, zs][slice_axis]
    dz, top = coords[1] - coords[0], coords[-1] + (coords[1] - coords[0])
    rng = np.random.default_rng(5)
    n = 9
    pos = rng.random((n, 3)) * [xs[-1], ys[-1], zs[-1]]
    pos[:, slice_axis] = (R + 1) * dz + rng.random(n) * (top - 2 * (R + 1) * dz)
    Z = rng.choice([6, 14, 79], n)
    got = pj.finite_potential(xs, ys, zs, pos, Z, R, J, slice_axis).sum(axis=2)
    want = orc.potential(xs, ys, zs, pos, Z, slice_axis).sum(axis=2)
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-12


def test_an_atom_on_a_node_is_one_partial_atom(pj):
    """w = 0: no second partial atom, and with R >= nz nothing folded inside the stack -- the exact slab potential"""
    xs, ys, zs = _grid(nz=6)
    J = 4
    e0, h = zs[0] - 0.25, 0.5 / J
    pos = np.array([[1.1, 0.9, e0 + 11 * h], [2.0, 1.7, e0 + 4 * h]])       # a node inside a slab, and a slab edge
    got = pj.finite_potential(xs, ys, zs, pos, [14, 79], 7, J)
    want = pj.exact_slab_potential(xs, ys, zs, pos, [14, 79])
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-13
    calls = []
    orig = pj.finite_form_factor
    try:
        pj.finite_form_factor = lambda Z, k2, a, b: (calls.append((Z, a, b)), orig(Z, k2, a, b))[1]
        pj.finite_potential(xs, ys, zs, pos[:1], [14], 1, J)
    finally:
        pj.finite_form_factor = orig
    assert len(calls) == 3                                      # one node x (2 R + 1) slabs; a second partial atom would make 6


def test_z_centroid_follows_the_atom(pj, orc):
    """one atom stepped through a slab in 16 steps: the centroid over the slices of its projected charge moves with it, where the
    infinite projection gives a staircase"""
    xs, ys, zs = _grid(nx=8, ny=8, nz=16)
    dz = 0.5
    z0 = zs[7] - dz / 2                                          # lower edge of slab 7
    steps = z0 + (np.arange(16) + 0.5) * dz / 16
    fin, inf = [], []
    for z in steps:
        pos = np.array([[1.0, 1.0, z]])
        for out, V in ((fin, pj.finite_potential(xs, ys, zs, pos, [79], 3, 4)), (inf, orc.potential(xs, ys, zs, pos, [79]))):
            q = V.sum(axis=(0, 1))
            out.append(float((q * zs).sum() / q.sum()))
    fin, inf = np.array(fin), np.array(inf)
    assert np.all(np.diff(inf) == 0.0) and abs(inf[0] - zs[7]) < 1e-12       # the staircase: the slice coordinate, whatever z is
    assert np.all(np.diff(fin) > 0.0)
    # the two partial atoms keep the centroid exactly; binning each node's symmetric profile on slabs it is not centred in moves it by
    # less than the node spacing h = dz / 4, the z resolution the model states
    assert np.max(np.abs(fin - steps)) < dz / 4, np.max(np.abs(fin - steps))


def test_convergence_in_the_node_count(pj):
    """|finite_potential - exact_slab_potential| falls monotonically over J = 1, 2, 4, 8 at a reach beyond the stack (DESIGN.md section
    4.26 records the values)"""
    xs, ys, zs = _grid(nx=12, ny=12, nz=8)
    rng = np.random.default_rng(11)
    pos = rng.random((6, 3)) * [xs[-1], ys[-1], 3.0] + [0, 0, 0.5]
    Z = [6, 14, 79, 6, 14, 79]
    exact = pj.exact_slab_potential(xs, ys, zs, pos, Z)
    errs = [np.linalg.norm(pj.finite_potential(xs, ys, zs, pos, Z, 9, J) - exact) / np.linalg.norm(exact) for J in (1, 2, 4, 8)]
    print("convergence J = 1, 2, 4, 8:", errs)
    assert errs[0] > errs[1] > errs[2] > errs[3] > 0.0


# ---- API ----------------------------------------------------------------------------------------------------------------------------

def test_projection_validation(pj):
    p = pj.Projection()
    assert (p.reach, p.nodes) == (2.0, 4)
    for bad in (dict(reach=0.0), dict(reach=-1.0), dict(reach=float("nan")), dict(reach="2"), dict(nodes=0), dict(nodes=17), dict(nodes=2.5),
                dict(nodes=True)):
        with pytest.raises(ValueError, match="Projection"):
            pj.Projection(**bad)
    assert pj.as_projection(None) is None and pj.as_projection("infinite") is None
    assert isinstance(pj.as_projection("finite"), pj.Projection) and pj.as_projection(p) is p
    for bad in ("Finite", 2.0, True):
        with pytest.raises(ValueError, match="projection"):
            pj.as_projection(bad)


def test_reach_in_slices(pj):
    assert pj.Projection(2.0).reach_slices(0.5) == 4
    assert pj.Projection(2.0).reach_slices(0.6) == 4
    assert pj.Projection(2.0).reach_slices(1.0) == 2
    assert pj.Projection(0.1).reach_slices(0.5) == 1
    assert pj.Projection(2.0).reach_slices(2.0 / 3.0) == 3                    # not 4 by a rounding of the quotient
    with pytest.raises(ValueError, match="more than 32"):
        pj.Projection(20.0).reach_slices(0.5)


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


def _trajectory(n_frames=2):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def test_constructor_refusals():
    from pyslice_amd import Detector, Projection
    for kw, name in ((dict(cache=True), "cache"), (dict(stream_tile=2), "stream_tile"),
                     (dict(tds=True, detectors=[Detector("haadf", inner=60.0, outer=200.0)]), "tds")):
        for proj in (Projection(), "finite"):
            with pytest.raises(ValueError, match=f"projection cannot be combined with {name}"):
                _calc(projection=proj, **kw)
        _calc(projection=None, **kw)
        _calc(projection="infinite", **kw)
    with pytest.raises(ValueError, match="projection"):
        _calc(projection=1.5)


def test_setup_refusals(monkeypatch):
    from pyslice_amd import AbsorptivePotential, _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("device work before the check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    tr = _trajectory(1)
    ap = AbsorptivePotential([int(z) for z in tr.atom_types], tr.positions[0], tr.box_matrix, 0.08)
    with pytest.raises(ValueError, match="projection cannot be combined with an AbsorptivePotential"):
        _calc(projection="finite").setup(ap, aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="projection cannot be combined with a run over several ranks"):
        _calc(projection="finite").setup(_trajectory(), aperture=30.0, voltage_eV=100e3, probe_positions=PP)


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)


def test_set_projection_once_before_the_first_build(recorder):
    from pyslice_amd import Projection
    calc = _calc(projection=Projection(reach=1.2, nodes=3))
    calc.setup(_trajectory(3), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    assert calc.projection_slices == 3 and calc.projection_node_spacing == pytest.approx((calc.zs[1] - calc.zs[0]) / 3)
    assert calc.projection_slices == int(np.ceil(1.2 / (calc.zs[1] - calc.zs[0])))
    calc.run()
    names = [c[0] for c in calc._engine.calls]
    assert names.count("set_projection") == 1
    i = names.index("set_projection")
    assert calc._engine.calls[i][1] == (3, 3)
    first_build = min(names.index(n) for n in ("build_potential", "build_potentials") if n in names)
    assert i < first_build
    # off: no call at all
    calc = _calc()
    calc.setup(_trajectory(2), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    calc.run()
    assert "set_projection" not in [c[0] for c in calc._engine.calls]
    assert calc.projection_slices is None and calc.projection_node_spacing is None


def test_slice_axis_with_other_spacing_is_refused(recorder):
    calc = _calc(projection="finite")
    with pytest.raises(ValueError, match="projection: slice_axis=0"):
        calc.setup(_trajectory(2), aperture=30.0, voltage_eV=100e3, probe_positions=PP, slice_axis=0)


def test_header_and_binding_symbols():
    from pyslice_amd import _native
    header = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"#define MSL_ABI_VERSION 3\b", header) and _native.ABI_VERSION == 3
    assert re.search(r"int\s+msl_set_projection\(msl_handle\* h, int32_t reach_slices, int32_t nodes\);", header)
    assert re.search(r"int\s+msl_get_projection\(const msl_handle\* h, int32_t\* reach_nodes\);", header)
    assert re.search(r"MSL_BUF_FORMFACTOR_FINITE = 17\b", header) and _native.BUF_FORMFACTOR_FINITE == 17
    assert "msl_set_projection" in _native.EXPORTS and "msl_get_projection" in _native.EXPORTS
    assert header.index("int  msl_set_projection(") > header.index("int  msl_fft2_host(")          # appended, nothing moved
    for name in ("set_projection", "get_projection", "form_factors_finite"):
        assert callable(getattr(_native.Engine, name))
