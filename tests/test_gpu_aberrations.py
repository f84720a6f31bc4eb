"""Aberrated probes on the MI355X: the device probe (probe_kspace_aberr_kernel + inverse FFT) against a float64 NumPy construction
from Aberrations.chi, the reference's defocus goldens, and the run modes that build their probes through msl_set_probes.

Bounds: 5e-6 relative L2 for a probe is the bound test_g10_probe_defocus uses for the same arrays; it does not depend on the size of
the aberration because the phase is reduced to one turn in float64 before the float32 sincos.  Exit waves: the 1e-4 of
test_gpu_parity.py.  Probe batches: the 1e-6 of the un-aberrated batch tests in test_gpu_detectors.py / test_gpu_diffraction.py."""
import math

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

PROBE_TOL = 5e-6
WAVE_TOL = 1e-4
ORDER = ["C10", "C12", "C21", "C23", "C30", "C32", "C34", "C41", "C43", "C45", "C50", "C52", "C54", "C56"]
# phase of each term at the aperture edge (30 mrad), rad: all inside 1 ... 50
EDGE_RAD = [40.0, 7.0, 12.0, 5.0, 50.0, 9.0, 4.0, 15.0, 6.0, 3.0, 25.0, 8.0, 5.0, 2.0]
MRAD, EV = 30.0, 100e3


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def grids(golden):
    g = golden("g10_defocus")
    return {"64": (g["xs_64"], g["ys_64"]), "96x80": (g["xs_96x80"], g["ys_96x80"]),
            "75x63": (np.arange(75) * 0.1, np.arange(63) * 0.11)}


def numpy_probes(ps, xs, ys, mrad, eV, ab, positions=((0.0, 0.0),)):
    """(P, nx, ny) complex128: ifft2(mask * centre-ramp * position-ramp * exp(-i chi)) in float64"""
    nx, ny = len(xs), len(ys)
    lam = ps.wavelength(eV)
    kx = np.fft.fftfreq(nx, xs[1] - xs[0])[:, None]
    ky = np.fft.fftfreq(ny, ys[1] - ys[0])[None, :]
    mask = np.hypot(kx, ky) < mrad * 1e-3 / lam
    fx = np.fft.fftfreq(nx, 1.0 / nx)[:, None]
    fy = np.fft.fftfreq(ny, 1.0 / ny)[None, :]
    centre = np.exp(2j * np.pi * (fx * (nx // 2) / nx + fy * (ny // 2) / ny))
    lens = np.exp(-1j * ab.chi(kx, ky, lam)) if ab is not None else 1.0
    out = [np.fft.ifft2(mask * centre * np.exp(2j * np.pi * (kx * px + ky * py)) * lens) for px, py in positions]
    return np.array(out)


def term(ps, i, scale=1.0):
    """term i alone: EDGE_RAD[i] * scale rad at the aperture edge, at an angle that is no multiple of pi / m"""
    name = ORDER[i]
    n, m = int(name[1]), int(name[2])
    lam = ps.wavelength(EV)
    kw = {name: scale * EDGE_RAD[i] * (n + 1) * lam / (2 * np.pi * (MRAD * 1e-3) ** (n + 1))}
    if m:
        phi = (i % 3 + 0.37) * math.pi / m
        assert min(abs(phi - j * math.pi / m) for j in range(2 * m + 1)) > 0.15
        kw["phi" + name[1:]] = phi
    return kw


def all_terms(ps):
    kw = {}
    for i in range(14):
        kw.update(term(ps, i, scale=-1.0 if i % 3 == 1 else 1.0))
    return ps.Aberrations(**kw)


def positions_for(xs, ys, seed=3, P=4):
    rng = np.random.default_rng(seed)
    return [tuple(v) for v in rng.random((P, 2)) * [len(xs) * (xs[1] - xs[0]), len(ys) * (ys[1] - ys[0])]]


# ------------------------------------------------------------------ 1. none / zero: the plain kernel, bit for bit
@pytest.mark.parametrize("tag", ["64", "96x80", "75x63"])
def test_zero_aberrations_are_bitwise_the_plain_probe(ps, golden, tag):
    from pyslice_amd import _native
    xs, ys = grids(golden)[tag]
    pp = positions_for(xs, ys)
    eng = _native.Engine(len(xs), len(ys), 1, xs[1] - xs[0], ys[1] - ys[0], 0.5, ps.wavelength(EV), 0.0, n_probes=len(pp), n_frames=0)
    try:
        eng.set_probes(MRAD, pp)
        plain = eng.probes()
        eng.set_aberrations(ps.Aberrations(Cs=1e7, defocus=-500.0))
        eng.set_probes(MRAD, pp)
        assert not np.array_equal(eng.probes(), plain)                        # (the state is read by set_probes)
        for ab in (None, ps.Aberrations(), ps.Aberrations(phi12=0.4, phi45=1.0)):
            eng.set_aberrations(ps.Aberrations(Cs=1e7))
            eng.set_aberrations(ab)
            eng.set_probes(MRAD, pp)
            assert np.array_equal(eng.probes(), plain)
        # the library's own argument checks
        polar = np.zeros((14, 2))
        assert eng._lib.msl_set_aberrations(eng._h, polar.ctypes.data, 13) == _native.MSL_ERR_INVALID
        assert eng._lib.msl_set_aberrations(eng._h, None, 14) == _native.MSL_ERR_INVALID
        for bad in (np.nan, np.inf):
            polar[5, 1] = bad
            assert eng._lib.msl_set_aberrations(eng._h, polar.ctypes.data, 14) == _native.MSL_ERR_INVALID
        eng.set_probes(MRAD, pp)                                              # a refused call leaves the state alone
        assert np.array_equal(eng.probes(), plain)
    finally:
        eng.close()
    base = npy(ps.Probe(xs, ys, MRAD, EV).array)
    assert np.array_equal(npy(ps.Probe(xs, ys, MRAD, EV, aberrations=ps.Aberrations()).array), base)
    assert np.array_equal(npy(ps.Probe(xs, ys, MRAD, EV, aberrations=None).array), base)
    # plane waves: chi(0) = 0, nothing changes
    pw = ps.create_batched_probes(ps.Probe(xs, ys, 0, EV), pp)
    pw_ab = ps.create_batched_probes(ps.Probe(xs, ys, 0, EV, aberrations=ps.Aberrations(Cs=1e7)), pp)
    assert np.array_equal(npy(pw_ab.array), npy(pw.array))


# ------------------------------------------------------------------ 2. defocus against the reference's goldens
@pytest.mark.parametrize("tag", ["64", "96x80"])
@pytest.mark.parametrize("dz", [100.0, 1000.0])
def test_defocus_matches_the_reference_goldens(ps, golden, tag, dz):
    g = golden("g10_defocus")
    pr = ps.Probe(g[f"xs_{tag}"], g[f"ys_{tag}"], float(g["mrad"]), float(g["eV"]), aberrations=ps.Aberrations(defocus=dz))
    got = npy(pr.array)
    err = rel_l2(got, g[f"defocus_{tag}_{dz:g}"])
    print(f"grid {tag} defocus {dz:g}: rel-L2 {err:.3e}")
    assert got.shape == g[f"defocus_{tag}_{dz:g}"].shape and got.dtype == np.complex128
    assert err < PROBE_TOL


# ------------------------------------------------------------------ 3. every term alone, then all together
def _check_on_all_grids(ps, golden, ab, label):
    worst = 0.0
    for tag, (xs, ys) in grids(golden).items():
        pp = positions_for(xs, ys, seed=len(tag))
        got = npy(ps.create_batched_probes(ps.Probe(xs, ys, MRAD, EV, aberrations=ab), pp).array)
        want = numpy_probes(ps, xs, ys, MRAD, EV, ab, pp)
        plain = numpy_probes(ps, xs, ys, MRAD, EV, None, pp)
        assert got.shape == want.shape
        errs = [rel_l2(got[p], want[p]) for p in range(len(pp))]
        print(f"{label} grid {tag}: max rel-L2 {max(errs):.3e} (aberrated vs plain {rel_l2(want, plain):.2e})")
        assert rel_l2(want, plain) > 0.05                  # the term is visibly on in the construction the device is held to
        worst = max(worst, max(errs))
        # 5. |exp(-i chi)| = 1: the intensity of the probe is that of the plain one
        s_ab, s_plain = (np.abs(got) ** 2).sum(axis=(1, 2)), (np.abs(plain) ** 2).sum(axis=(1, 2))
        assert np.allclose(s_ab, s_plain, rtol=1e-5, atol=0)
        base = npy(ps.Probe(xs, ys, MRAD, EV, aberrations=ab).array)             # the single probe at the origin
        assert base.ndim == 2 and rel_l2(base, numpy_probes(ps, xs, ys, MRAD, EV, ab)[0]) < PROBE_TOL
    assert worst < PROBE_TOL, (label, worst)


@pytest.mark.parametrize("i", range(14), ids=ORDER)
def test_one_term_at_a_time(ps, golden, i):
    _check_on_all_grids(ps, golden, ps.Aberrations(**term(ps, i)), ORDER[i])


def test_all_terms_together(ps, golden):
    _check_on_all_grids(ps, golden, all_terms(ps), "all fourteen")


def test_large_spherical_aberration_keeps_the_bound(ps, golden):
    """Cs = 1 mm: 344 rad at the aperture edge; with Scherzer-like defocus.  The float64 reduction keeps the fp32 error where it is."""
    _check_on_all_grids(ps, golden, ps.Aberrations(Cs=1e7, defocus=ps.scherzer_defocus(1e7, EV)), "Cs 1 mm + Scherzer")


# ------------------------------------------------------------------ 6. through the run modes
@pytest.fixture(scope="module")
def small_run(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 6, 2, density=0.2, seed=1)
    ab = ps.Aberrations(defocus=-150.0, Cs=2e6, astigmatism=60.0, astigmatism_angle=0.4, coma=3000.0, coma_angle=1.3)
    return tr, ab


def test_calculator_run_equals_propagate_with_numpy_probes(ps, small_run):
    tr, ab = small_run
    pp = [(3.0, 3.0), (1.2, 4.4), (5.1, 0.7)]
    calc = ps.MultisliceCalculator(progress=False, aberrations=ab)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    xs, ys, zs = calc.xs, calc.ys, calc.zs
    probes = numpy_probes(ps, xs, ys, MRAD, EV, ab, pp)
    plain = ps.MultisliceCalculator(progress=False)
    plain.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    off = npy(plain.run().wavefunction_data)
    for t in range(tr.n_frames):
        pot = ps.Potential(xs, ys, zs, tr.positions[t], list(tr.atom_types))
        ex = npy(ps.Propagate(ps.Probe(xs, ys, MRAD, EV, array=probes), pot))
        want = np.fft.fftshift(np.fft.fft2(ex), axes=(-2, -1))
        err = rel_l2(got[:, t, :, :, 0], want)
        print(f"frame {t}: run() vs Propagate(numpy probes) rel-L2 {err:.3e}; aberrated vs plain {rel_l2(got[:, t], off[:, t]):.2e}")
        assert err < WAVE_TOL
        assert rel_l2(got[:, t], off[:, t]) > 100 * WAVE_TOL
        # the analytic recipe through Propagate: the same probes, built on the potential's engine
        ex2 = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(xs, ys, MRAD, EV, aberrations=ab), pp), pot))
        assert rel_l2(ex2, ex) < WAVE_TOL


def _scan(ps, tr, n=19):
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    return [tuple(v) for v in np.random.default_rng(22).random((n, 2)) * [lx, ly]]


def test_detector_runs_with_aberrations_over_probe_batches(ps, small_run):
    tr, ab = small_run
    pp = _scan(ps, tr)
    D = ps.Detector
    dets = [D("bf", outer=MRAD), D("abf", inner=MRAD / 2, outer=MRAD), D("adf", inner=1.5 * MRAD, outer=150.0),
            D("dpc0", outer=MRAD, azimuth=(0.0, 90.0)), D("comx", signal="com_x"), D("comy", signal="com_y"),
            D("haadf", inner=1.5 * MRAD, signal="amplitude")]
    out = {}
    for key, a, pb in (("all", ab, 19), ("7", ab, 7), ("plain", None, 19)):
        calc = ps.MultisliceCalculator(progress=False, detectors=dets, probe_batch=pb, frame_batch=2, aberrations=a)
        calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
        assert calc.probe_batch == pb
        out[key] = calc.run_detectors().signals
    scale = np.abs(out["all"]).max(axis=(0, 1), keepdims=True)
    same = (np.abs(out["7"] - out["all"]) / scale).max()
    on = (np.abs(out["plain"] - out["all"]) / scale).max()
    print(f"detectors: probe_batch 7 vs 19 max diff / scale {same:.3e}; aberrated vs plain {on:.3e}")
    assert same <= 1e-6
    assert on > 1e-3


def test_diffraction_runs_with_aberrations_over_probe_batches(ps, small_run):
    tr, ab = small_run
    pp = _scan(ps, tr)
    out = {}
    for key, a, pb in (("all", ab, 19), ("7", ab, 7), ("plain", None, 19)):
        calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=(2, 4)), probe_batch=pb, frame_batch=2, aberrations=a)
        calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
        out[key] = calc.run_diffraction().intensity
    scale = out["all"].max(axis=(-2, -1), keepdims=True)
    same = (np.abs(out["7"] - out["all"]) / scale).max()
    on = (np.abs(out["plain"] - out["all"]) / scale).max()
    print(f"diffraction: probe_batch 7 vs 19 max diff / pattern max {same:.3e}; aberrated vs plain {on:.3e}")
    assert same <= 1e-6
    assert on > 1e-3


# ------------------------------------------------------------------ 7. the state on a shared engine
def test_propagate_clears_the_aberrations_of_the_previous_probe(ps, small_run):
    tr, ab = small_run
    xs, ys, zs, *_ = ps.gridFromTrajectory(tr)
    pp = [(3.0, 3.0), (1.2, 4.4)]
    fresh = ps.Potential(xs, ys, zs, tr.positions[0], list(tr.atom_types))
    want = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(xs, ys, MRAD, EV), pp), fresh))
    pot = ps.Potential(xs, ys, zs, tr.positions[0], list(tr.atom_types))
    first = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(xs, ys, MRAD, EV, aberrations=ab), pp), pot))
    second = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(xs, ys, MRAD, EV), pp), pot))
    assert rel_l2(first, want) > 100 * WAVE_TOL
    assert np.array_equal(second, want)
