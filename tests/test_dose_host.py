"""Finite dose on the host: the Dose request, the refusals, the ABI tables, DiffractionData on counts, and the definition of the
Poisson draw (pyslice_amd/dose.py) -- exactness and statistics.  Fixed seeds: every statement is deterministic."""
import math
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


def _raster(nx=4, ny=3, sx=0.5, sy=0.25):
    return [(1.0 + i * sx, 2.0 + j * sy) for i in range(nx) for j in range(ny)]


# ------------------------------------------------------------------ 1. the request
def test_dose_validation():
    from pyslice_amd import Dose
    assert Dose(electrons_per_probe=1e4).electrons_per_probe == 1e4
    d = Dose(per_area=100.0, seed=7, keep_intensity=True)
    assert (d.per_area, d.seed, d.keep_intensity, d.electrons_per_probe) == (100.0, 7, True, None)
    assert Dose(electrons_per_probe=0).electrons_per_probe == 0.0
    for kw in (dict(), dict(electrons_per_probe=1.0, per_area=1.0), dict(electrons_per_probe=-1.0), dict(electrons_per_probe=float("nan")),
               dict(per_area=float("inf")), dict(electrons_per_probe="many"), dict(electrons_per_probe=True),
               dict(electrons_per_probe=1.0, seed=-1), dict(electrons_per_probe=1.0, seed=1.5), dict(electrons_per_probe=1.0, seed=2 ** 64),
               dict(electrons_per_probe=1.0, keep_intensity=1)):
        with pytest.raises(ValueError):
            Dose(**kw)
    assert Dose(electrons_per_probe=1.0, seed=2 ** 64 - 1).seed == 2 ** 64 - 1


def test_per_area_on_regular_and_irregular_scans():
    from pyslice_amd import Dose
    d = Dose(per_area=1000.0)
    assert d.electrons(_raster()) == pytest.approx(1000.0 * 0.5 * 0.25, rel=1e-12)
    assert Dose(electrons_per_probe=50.0).electrons([(0.3, 0.1), (5.0, 2.2), (1.0, 1.0)]) == 50.0
    rng = np.random.default_rng(1)
    for bad in ([tuple(v) for v in rng.random((12, 2))],              # random positions
                _raster()[:-1],                                        # a raster with a hole
                [(0.0, 0.0), (1.0, 0.0), (3.0, 0.0), (0.0, 1.0), (1.0, 1.0), (3.0, 1.0)],      # uneven steps
                [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)],                  # one row: no area
                [(1.0, 1.0)]):
        with pytest.raises(ValueError, match="per_area"):
            d.electrons(bad)


def test_setup_resolves_per_area_before_device_work(traj, monkeypatch):
    from pyslice_amd import Diffraction, Dose, _native

    def no_engine(*a, **k):
        raise AssertionError("device work before the dose check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = _calc(diffraction=Diffraction(dose=Dose(per_area=10.0)))
    with pytest.raises(ValueError, match="per_area"):
        calc.setup(traj, aperture=30.0, voltage_eV=100e3, probe_positions=[(1.0, 1.0), (2.0, 3.0), (2.5, 0.5)])
    assert calc._engine is None


# ------------------------------------------------------------------ 2. refusals
def test_refusals_in_the_constructor():
    from pyslice_amd import Detector, Diffraction, Dose, PolarDetector, Precession, Thickness
    from pyslice_amd.prism import Prism
    dose = Dose(electrons_per_probe=1e3)
    with pytest.raises(NotImplementedError, match=r"dose: split=True is not built"):
        Diffraction(split=True, dose=dose)
    with pytest.raises(ValueError, match="Dose"):
        Diffraction(dose=1e3)
    d = Diffraction(bin=(2, 2), dose=dose)
    for what, kw in (("thickness", dict(thickness=Thickness(every=2))), ("prism", dict(prism=Prism((2, 2)))),
                     ("precession", dict(precession=Precession(10.0, 4))), ("polar", dict(polar=PolarDetector(outer=40.0))),
                     ("cache", dict(cache=True)), ("stream_tile", dict(stream_tile=4))):
        with pytest.raises(NotImplementedError, match=rf"dose: {what} is not built"):
            _calc(diffraction=d, **kw)
    _calc(diffraction=d, k_window=(16, 16), probe_batch=3, frame_batch=2, detectors=[Detector("bf", outer=10.0)])      # carried


def test_several_ranks_refused_in_setup(traj, monkeypatch):
    from pyslice_amd import Diffraction, Dose, _native, distributed
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))

    def no_engine(*a, **k):
        raise AssertionError("device work before the rank check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    calc = _calc(diffraction=Diffraction(dose=Dose(electrons_per_probe=10.0)))
    with pytest.raises(NotImplementedError, match=r"dose: several ranks is not built"):
        calc.setup(traj, aperture=30.0, voltage_eV=100e3)
    assert calc._engine is None


# ------------------------------------------------------------------ 3. the ABI tables
def test_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    main = open(os.path.join(REPO, "pyslice_amd", "csrc", "mslice.hip")).read()
    for name in ("msl_dose_reset", "msl_dose_add", "msl_dose_counts"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert re.search(rf"\bint {name}\s*\(", main), name
        assert name in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr) and _native.ABI_VERSION == 3
    for method in ("dose_reset", "dose_add", "dose_counts"):
        assert callable(getattr(_native.Engine, method))
    # the Philox round function exists once: dose.h takes thermal.h's
    dose_h = open(os.path.join(REPO, "pyslice_amd", "csrc", "dose.h")).read()
    assert '#include "thermal.h"' in dose_h and "0xD2511F53" not in dose_h


# ------------------------------------------------------------------ 4. the data classes
def test_stem_and_polar_poisson():
    from pyslice_amd import Detector, PolarData, PolarDetector, Probe, STEMData
    from pyslice_amd.dose import incident_intensity, poisson_counts, probe_incident
    xs, ys = np.arange(48) * 0.1, np.arange(40) * 0.1
    probe = Probe(xs, ys, 30.0, 100e3)
    inc = probe_incident(probe)
    assert inc == incident_intensity(48, 40, 0.1, 0.1, 30.0, probe.wavelength) and inc > 20
    kx = np.fft.fftshift(np.fft.fftfreq(48, 0.1))
    ky = np.fft.fftshift(np.fft.fftfreq(40, 0.1))
    rng = np.random.default_rng(5)
    pp = _raster()
    sig = rng.random((len(pp), 3, 2)) * inc
    dets = [Detector("bf", outer=30.0), Detector("adf", inner=40.0, outer=100.0)]
    st = STEMData(signals=sig, detectors=dets, probe_positions=pp, time=np.arange(3.0), kxs=kx, kys=ky, probe=probe)
    c = st.poisson(1e4, seed=3)
    assert c.shape == (len(pp), 2) and c.dtype == np.uint32
    assert np.array_equal(c, poisson_counts(sig.mean(axis=1) * (1e4 / inc), 3, np.arange(len(pp))))
    assert abs(c.sum() / (sig.mean(axis=1).sum() * 1e4 / inc) - 1) < 0.01
    for signal in ("amplitude", "com_x", "com_y"):
        bad = STEMData(signals=sig, detectors=[dets[0], Detector("x", signal=signal)], probe_positions=pp, time=np.arange(3.0),
                       kxs=kx, kys=ky, probe=probe)
        with pytest.raises(ValueError, match="intensity"):
            bad.poisson(1e4)
    pol = PolarDetector(outer=40.0, step=10.0, n_azimuthal=2)
    ps = rng.random((len(pp), 4, 2)) * inc
    pd = PolarData(signals=ps, polar=pol, counts=np.ones((4, 2), dtype=np.int64), edges=pol.edges, probe_positions=pp,
                   time=np.arange(3.0), kxs=kx, kys=ky, probe=probe)
    from pyslice_amd import Dose
    cp = pd.poisson(Dose(per_area=8e4, seed=9))
    assert cp.shape == ps.shape and np.array_equal(cp, poisson_counts(ps * (8e4 * 0.125 / inc), 9, np.arange(len(pp))))


def _counted(keep=True, P=12, shape=(8, 6)):
    from pyslice_amd import DiffractionData, Dose
    rng = np.random.default_rng(2)
    kx = np.fft.fftshift(np.fft.fftfreq(shape[0], 0.1)).astype(np.float32)
    ky = np.fft.fftshift(np.fft.fftfreq(shape[1], 0.1)).astype(np.float32)
    counts = rng.integers(0, 50, size=(P,) + shape).astype(np.uint32)
    inten = rng.random((P,) + shape)
    return DiffractionData(intensity=inten if keep else None, kxs=kx, kys=ky, bin=(1, 1), n_frames=3, probe_positions=_raster(),
                           probe=None, wavelength=0.037, counts=counts, dose=Dose(electrons_per_probe=100.0),
                           electrons_per_probe=100.0, incident=30.0), counts, inten


def test_diffraction_data_on_counts():
    from pyslice_amd import Detector, DiffractionData
    dd, counts, _ = _counted(keep=False)
    assert dd.intensity is None and dd.counts.dtype == np.uint32
    assert np.array_equal(dd.pacbed(), counts.astype(np.float64).mean(axis=0)) and dd.pacbed().dtype == np.float64
    det = Detector("bf", outer=60.0)
    m = dd.member(det)
    assert m.any() and not m.all()
    assert np.array_equal(dd.virtual(det), (counts * m[None]).sum(axis=(-2, -1)).astype(np.float64))
    assert dd.image(det).shape == (4, 3)
    assert np.array_equal(dd.pattern(1.0, 2.0), counts[0].astype(np.float64))
    with pytest.raises(ValueError, match="keep_intensity"):
        dd.pacbed(part="intensity")
    with pytest.raises(ValueError, match="part"):
        dd.pacbed(part="total")
    both, counts, inten = _counted(keep=True)
    assert np.array_equal(both.pacbed(), inten.mean(axis=0))           # today's behaviour while there is an intensity
    assert np.array_equal(both.pacbed(part="counts"), counts.astype(np.float64).mean(axis=0))
    assert np.array_equal(both.virtual(det, part="intensity"), both.virtual(det))
    assert np.array_equal(both.pattern(1.0, 2.0, part="counts"), counts[0].astype(np.float64))
    plain = DiffractionData(intensity=inten, kxs=both.kxs, kys=both.kys, bin=(1, 1), n_frames=3, probe_positions=_raster(), probe=None,
                            wavelength=0.037)
    assert plain.counts is None and plain.dose is None and np.array_equal(plain.pacbed(), inten.mean(axis=0))
    with pytest.raises(ValueError, match="dose"):
        plain.pacbed(part="counts")
    with pytest.raises(ValueError):
        DiffractionData(intensity=None, kxs=both.kxs, kys=both.kys, bin=(1, 1), n_frames=3, probe_positions=_raster(), probe=None)
    with pytest.raises(ValueError, match="shape"):
        DiffractionData(intensity=inten[:, :4], kxs=both.kxs, kys=both.kys, bin=(1, 1), n_frames=3, probe_positions=_raster(),
                        probe=None, wavelength=0.037, counts=counts)


# ------------------------------------------------------------------ 5. the definition: exactness
def test_uniforms_are_odd_multiples_of_2_to_minus_53():
    from pyslice_amd.dose import _uniform53
    hi = np.array([0, 0xFFFFFFFF, 0x80000000, 63], dtype=np.uint32)
    lo = np.array([0, 0xFFFFFFFF, 0, 63], dtype=np.uint32)
    u = _uniform53(hi, lo)
    assert u[0] == 2.0 ** -53 and u[1] == 1.0 - 2.0 ** -53 and u[2] == 0.5 + 2.0 ** -53 and u[3] == 2.0 ** -53
    assert np.all((u * 2.0 ** 53) % 2 == 1)


def test_counts_are_a_pure_function_of_seed_probe_and_pixel():
    from pyslice_amd.dose import poisson_counts
    rng = np.random.default_rng(8)
    lam = np.concatenate([rng.random((5, 300)) * 9.0, rng.random((5, 300)) * 300.0 + 10.0], axis=1).reshape(5, 20, 30)
    probes = np.array([0, 1, 2, 7, 2 ** 32 - 1])
    a = poisson_counts(lam, 11, probes)
    assert a.dtype == np.uint32 and a.shape == lam.shape
    assert np.array_equal(a, poisson_counts(lam, 11, probes))
    # the split of the probes over calls, and their order, do not matter
    assert np.array_equal(a[:2], poisson_counts(lam[:2], 11, probes[:2]))
    assert np.array_equal(a[2:], poisson_counts(lam[2:], 11, probes[2:]))
    for j, p in enumerate(probes):
        assert np.array_equal(a[j], poisson_counts(lam[j], 11, int(p)))
    assert np.array_equal(a[::-1], poisson_counts(lam[::-1], 11, probes[::-1]))
    # the pixel index is the row-major index, whatever the shape
    assert np.array_equal(a[3].reshape(-1), poisson_counts(lam[3].reshape(-1), 11, 7))
    # other seeds and other probes give other draws
    assert (poisson_counts(lam, 12, probes) != a).mean() > 0.5
    assert (poisson_counts(lam, 11 + 2 ** 32, probes) != a).mean() > 0.5             # the high key word counts
    assert (poisson_counts(lam[0], 11, 1) != a[0]).mean() > 0.5


def test_zero_limits_and_errors():
    from pyslice_amd.dose import COUNT_MAX, K_LIMIT, poisson_counts
    assert not poisson_counts(np.zeros((3, 4)), 5, 0).any()
    lam = np.array([0.0, 1e-300, 1e-12, 5.0, 0.0, 80.0])
    c = poisson_counts(lam, 5, 0)
    assert c[0] == 0 and c[1] == 0 and c[2] == 0 and c[4] == 0 and c[5] > 30
    assert poisson_counts(np.full(1000, 9.99), 1, 0).max() <= K_LIMIT
    big = poisson_counts(np.array([1e12, 1e300, 4294967295.0 * 4]), 5, 3)
    assert np.all(big == COUNT_MAX)
    near = poisson_counts(np.full(100, 4.0e9), 5, 3).astype(np.float64)
    assert np.all(np.abs(near - 4.0e9) < 6 * math.sqrt(4.0e9))
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lam"):
            poisson_counts(np.array([1.0, bad]), 5, 0)
    with pytest.raises(ValueError):
        poisson_counts(np.ones((2, 3)), 5, [0, 1, 2])
    with pytest.raises(ValueError):
        poisson_counts(np.ones(3), 5, -1)
    with pytest.raises(ValueError):
        poisson_counts(np.ones(3), -5, 0)


# ------------------------------------------------------------------ 6. the definition: statistics
N_DRAWS = 200_000


@pytest.mark.parametrize("j,lam", list(enumerate([0.01, 0.5, 3.0, 9.999, 10.0, 50.0, 1e3, 1e6])))
def test_sampler_statistics(j, lam):
    """2e5 draws: mean and variance within 5 standard errors of lam (the variance of the sample variance of a Poisson variate is
    (lam + 2 lam^2 N / (N - 1)) / N), and the chi-square of the histogram against the pmf over the counts whose expectation is >= 5
    below the 1 - 1e-6 quantile of its degrees of freedom.  9.999 and 10 pin the inversion and the PTRS branch."""
    from scipy.stats import chi2
    from pyslice_amd.dose import poisson_counts
    k = poisson_counts(np.full(N_DRAWS, lam), 1234 + j, j).astype(np.int64)
    N = N_DRAWS
    mean, var = k.mean(), k.var(ddof=1)
    se_mean = math.sqrt(lam / N)
    se_var = math.sqrt((lam + 2.0 * lam * lam * N / (N - 1)) / N)
    lo, hi = int(k.min()), int(k.max())
    ks = np.arange(max(0, lo - 5), hi + 6)
    expect = N * np.exp(np.array([kk * math.log(lam) - lam - math.lgamma(kk + 1.0) for kk in ks]))
    seen = np.bincount(k - ks[0], minlength=ks.size)[:ks.size]
    use = expect >= 5.0
    stat = float((((seen - expect) ** 2) / expect)[use].sum())
    df = int(use.sum()) - 1
    bound = float(chi2.ppf(1.0 - 1e-6, df))
    print(f"lam {lam:g}: mean z {(mean - lam) / se_mean:+.2f}, variance z {(var - lam) / se_var:+.2f}, chi2 {stat:.1f} of {df} dof "
          f"(bound {bound:.1f})")
    assert df >= 1
    assert abs(mean - lam) <= 5.0 * se_mean
    assert abs(var - lam) <= 5.0 * se_var
    assert stat < bound
