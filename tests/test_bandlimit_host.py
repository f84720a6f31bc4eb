"""Band limit on the host: the cuts and masks of pyslice_amd/bandlimit.py, the alias-freeness of the float64 definition (the property
the feature exists for), its equality with the oracle's recursion where nothing is out of band, the refusals, the calls the
calculator makes on a recording engine, and the ABI."""
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine, format_calls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = [(0.3 * i, 0.2 * i) for i in range(5)]
LAM = 0.037                                     # Angstrom, about 100 keV


# ------------------------------------------------------------------ 1. cuts and masks
@pytest.mark.parametrize("nx,ny,dx,dy", [(64, 64, 0.1, 0.1), (96, 80, 0.11, 0.13), (501, 491, 0.1, 0.1), (33, 48, 0.2, 0.1),
                                         (96, 96, 0.125, 0.125)])
@pytest.mark.parametrize("fraction", [2.0 / 3.0, 0.5])
def test_cuts_are_strict_and_alias_free(nx, ny, dx, dy, fraction):
    from pyslice_amd.bandlimit import BandLimit, mask, mask_1d
    bl = BandLimit(fraction)
    kc = fraction * min(1.0 / (2 * dx), 1.0 / (2 * dy))
    assert bl.cutoff(dx, dy) == kc
    cx, cy = bl.cuts(nx, ny, dx, dy)
    for n, d, c in ((nx, dx, cx), (ny, dy, cy)):
        assert c >= 1 and 3 * c < n
        assert c / (n * d) < kc                                              # the largest kept index is inside, strictly
        assert (c + 1) / (n * d) >= kc or 3 * (c + 1) >= n                   # and the next one is not (or would alias)
        m = mask_1d(n, c)
        assert m.shape == (n,) and set(np.unique(m)) == {0.0, 1.0} and m.sum() == 2 * c + 1
        assert np.array_equal(m[1:], m[1:][::-1])                           # even in the signed index
        h = np.rint(np.fft.fftfreq(n) * n)
        assert np.array_equal(m, (np.abs(h) <= c).astype(float))
    assert np.array_equal(mask(nx, ny, cx, cy), mask_1d(nx, cx)[:, None] * mask_1d(ny, cy)[None, :])
    # the same physical cutoff on both axes, and the angle of the tighter axis
    assert abs(bl.max_angle_mrad(LAM, nx, ny, dx, dy) - 1e3 * LAM * min(cx / (nx * dx), cy / (ny * dy))) < 1e-12


def test_the_strict_edge():
    """64 points at fraction 0.5: kc n d = 16 exactly (powers of two, no rounding), and the test is strict: 16 is out"""
    from pyslice_amd.bandlimit import BandLimit
    assert BandLimit(0.5).cuts(64, 64, 0.125, 0.125) == (15, 15)
    assert BandLimit(0.5).cuts(64, 128, 0.125, 0.125) == (15, 31)            # isotropic in physical units
    assert BandLimit(0.5).cuts(64, 64, 0.125, 0.25) == (7, 15)               # the coarser axis sets kc
    # 2/3 of Nyquist on 96 points is index 32 in exact arithmetic: out, whatever the rounding of 2/3 does
    assert BandLimit().cuts(96, 96, 0.125, 0.125) == (31, 31)


def test_the_float64_edge_at_a_third_of_the_axis():
    """2/3 of Nyquist on the tighter axis of a length divisible by 3 puts h = n / 3 on the edge in exact arithmetic (out: the test is
    strict).  In float64 the comparison falls either way -- at d = 0.11 it keeps 49 of 147 -- and cuts() holds the alias-free bound."""
    from pyslice_amd.bandlimit import BandLimit
    bl = BandLimit()
    kc = bl.cutoff(0.11, 0.11)
    assert 49 / (147 * 0.11) < kc                                            # (the float64 test alone would keep h = 49 = n / 3)
    for n in (147, 153, 294, 306, 96, 99, 3198):
        for d in (0.11, 0.1, 0.125):
            c = bl.cuts(n, n, d, d)[0]
            assert c == (n - 1) // 3 and 3 * c < n, (n, d, c)                  # the largest h below n / 3


def test_bandlimit_values():
    from pyslice_amd.bandlimit import BandLimit, as_bandlimit
    for bad in (0.7, 0, 0.0, -0.1, float("nan"), float("inf"), True, "2/3", None):
        with pytest.raises(ValueError, match="BandLimit"):
            BandLimit(bad)
    assert BandLimit().fraction == 2.0 / 3.0 and BandLimit(0.5) == BandLimit(0.5) and BandLimit(0.5) != BandLimit()
    assert as_bandlimit(None) is None and as_bandlimit(0.5) == BandLimit(0.5) and as_bandlimit(BandLimit()) == BandLimit()
    with pytest.raises(ValueError, match="bandlimit"):
        as_bandlimit("x")
    with pytest.raises(ValueError, match="BandLimit"):
        BandLimit(0.01).cuts(16, 16, 0.1, 0.1)                               # keeps nothing but zero
    with pytest.raises(AttributeError):
        BandLimit().fraction = 0.5


# ------------------------------------------------------------------ 2. the definition
def _pad_spectrum(F, N0, N1):
    """zero-pad a spectrum in FFT order (.., n0, n1) to (.., N0, N1), index by signed index; scaled so that the padded field takes
    the values of the original at the coincident points.  The Nyquist bin of an even axis goes to -n/2, as numpy stores it."""
    n0, n1 = F.shape[-2:]
    out = np.zeros(F.shape[:-2] + (N0, N1), dtype=np.complex128)
    h0 = np.rint(np.fft.fftfreq(n0) * n0).astype(int)
    h1 = np.rint(np.fft.fftfreq(n1) * n1).astype(int)
    out[..., (h0 % N0)[:, None], (h1 % N1)[None, :]] = F
    return out * (N0 * N1) / (n0 * n1)


def _phase_object(nx, ny, nz, seed):
    """a smooth random phase object with strong phases: exp(i phi) has content far beyond the band"""
    rng = np.random.default_rng(seed)
    spec = (rng.standard_normal((nz, nx, ny)) + 1j * rng.standard_normal((nz, nx, ny)))
    hx, hy = np.fft.fftfreq(nx) * nx, np.fft.fftfreq(ny) * ny
    spec *= np.exp(-(hx[:, None] ** 2 + hy[None, :] ** 2) / 18.0)
    phi = np.fft.ifft2(spec).real
    return np.exp(1j * 6.0 * phi / np.abs(phi).max())


def test_the_definition_is_alias_free():
    """48 x 40 against 96 x 80 at half the sampling, fed the zero-padded spectra of the same limited t_k and masked psi0: inside the
    band the exit spectra agree to rounding -- nothing folded back on the small grid.  Without the limit they do not."""
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import BandLimit, bandlimit_transmission, mask, propagate_bandlimited
    nx, ny, nz, dx, dy, dz = 48, 40, 3, 0.2, 0.24, 2.0
    t = _phase_object(nx, ny, nz, seed=5)
    xs, ys = np.arange(nx) * dx, np.arange(ny) * dy
    psi0 = orc.batched_probes(orc.probe_array(xs, ys, 18.0, 100e3), xs, ys, [(4.1, 5.3)])
    cx, cy = BandLimit().cuts(nx, ny, dx, dy)
    M = mask(nx, ny, cx, cy)
    band = M.astype(bool)

    def pad(a):
        return np.fft.ifft2(_pad_spectrum(np.fft.fft2(a, axes=(-2, -1)), 2 * nx, 2 * ny), axes=(-2, -1))

    def in_band(exit_small, exit_big):
        a = np.fft.fft2(exit_small, axes=(-2, -1))[..., band]
        big = np.fft.fft2(exit_big, axes=(-2, -1)) / 4.0
        hx = np.rint(np.fft.fftfreq(nx) * nx).astype(int) % (2 * nx)
        hy = np.rint(np.fft.fftfreq(ny) * ny).astype(int) % (2 * ny)
        b = big[..., hx[:, None], hy[None, :]][..., band]
        return np.linalg.norm(a - b) / np.linalg.norm(b)

    # limited: the big grid gets the limited t_k and the masked psi0 (limiting them again there changes nothing: same cuts)
    tl = bandlimit_transmission(t, cx, cy)
    psim = np.fft.ifft2(M * np.fft.fft2(psi0, axes=(-2, -1)), axes=(-2, -1))
    small = propagate_bandlimited(psi0, t, dx, dy, LAM, dz, (cx, cy))
    big = propagate_bandlimited(pad(psim), pad(tl), dx / 2, dy / 2, LAM, dz, (cx, cy))
    err = in_band(small, big)
    assert err < 1e-10, err
    # masking psi0 first changes nothing in the band either: the first propagator removes what lies outside
    small_m = propagate_bandlimited(psim, t, dx, dy, LAM, dz, (cx, cy))
    assert in_band(small_m, big) < 1e-10
    # the limit off: the same comparison, with the unlimited factors padded -- the small grid aliases
    small0 = propagate_bandlimited(psi0, t, dx, dy, LAM, dz, None)
    big0 = propagate_bandlimited(pad(psi0), pad(t), dx / 2, dy / 2, LAM, dz, None)
    err0 = in_band(small0, big0)
    assert err0 > 1e-3, err0


def test_transmission_lowpass_is_a_projection():
    from pyslice_amd.bandlimit import bandlimit_transmission, mask
    t = _phase_object(30, 25, 2, seed=1)
    tl = bandlimit_transmission(t, 7, 6)
    assert tl.shape == t.shape and tl.dtype == np.complex128
    F = np.fft.fft2(tl, axes=(-2, -1))
    out = ~mask(30, 25, 7, 6).astype(bool)
    assert np.abs(F[:, out]).max() < 1e-12 * np.abs(F).max()
    assert np.allclose(bandlimit_transmission(tl, 7, 6), tl, rtol=0, atol=1e-14)
    assert np.allclose(bandlimit_transmission(t[0], 7, 6), tl[0], rtol=0, atol=1e-15)
    assert np.abs(tl - t).max() > 1e-3                                       # exp(i phi) was not band-limited


def test_limit_equals_the_oracle_recursion_when_nothing_is_out_of_band():
    """t_k synthesised inside |h| <= 2 and waves inside |h| <= 3 on 64 x 48 with cuts (20, 15): after two products the wave reaches
    |h| <= 7, far inside the cuts, so neither mask removes anything and the limited recursion is the oracle's plain one."""
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import mask, propagate_bandlimited
    nx, ny, nz, eV = 64, 48, 3, 100e3
    xs, ys, zs = np.arange(nx) * 0.1, np.arange(ny) * 0.12, np.arange(nz) * 0.5
    rng = np.random.default_rng(2)

    def field(shape, c):
        F = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * mask(nx, ny, c, c)
        return np.fft.ifft2(F, axes=(-2, -1)) * 20.0
    t = 1.0 + 0.3 * field((nz, nx, ny), 2)                                    # a complex field: not exp(i sigma V) of a real V,
    psi0 = field((2, nx, ny), 3)                                             # so the oracle's loop is fed log(t) / (i sigma)
    sig = orc.interaction_sigma(eV)
    V = np.moveaxis(np.log(t) / (1j * sig), 0, 2)
    want = orc.propagate(psi0, V, xs, ys, zs, eV)
    got = propagate_bandlimited(psi0, t, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(eV), zs[1] - zs[0], (20, 15))
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-12
    plain = propagate_bandlimited(psi0, t, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(eV), zs[1] - zs[0], None)
    assert np.linalg.norm(plain - want) / np.linalg.norm(want) < 1e-12
    with pytest.raises(ValueError, match="alias-free"):
        propagate_bandlimited(psi0, t, 0.1, 0.12, LAM, 0.5, (22, 15))        # 3 * 22 >= 64


def test_a_tilt_with_a_limit_is_a_masked_tilted_table():
    from pyslice_amd.bandlimit import bandlimit_transmission, mask, propagate_bandlimited
    from pyslice_amd.tilt import Tilt, tilted_propagator
    nx, ny, dx, dy, dz = 36, 30, 0.2, 0.21, 1.5
    t = _phase_object(nx, ny, 2, seed=3)
    psi0 = np.random.default_rng(1).standard_normal((1, nx, ny)) + 0j
    tilt = Tilt(20.0, -10.0)
    got = propagate_bandlimited(psi0, t, dx, dy, LAM, dz, (10, 9), tilt=tilt)
    P = tilted_propagator(nx, ny, dx, dy, LAM, dz, tilt) * mask(nx, ny, 10, 9)
    tl = bandlimit_transmission(t, 10, 9)
    want = tl[1] * np.fft.ifft2(P * np.fft.fft2(tl[0] * psi0))
    assert np.allclose(got, want, rtol=0, atol=1e-13)


# ------------------------------------------------------------------ 3. the calculator on a recording engine
def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def _dets():
    from pyslice_amd import Detector
    return [Detector("bf", outer=20.0), Detector("adf", inner=40.0, outer=120.0)]


def _setup(calc, n_frames=2, aperture=30.0, **kw):
    calc.setup(_trajectory(n_frames), aperture=aperture, voltage_eV=100e3, probe_positions=PP, **kw)
    return calc


class Engine(RecordingEngine):
    """the recording engine, with an answer for the polar detector's read as well"""

    def __getattr__(self, name):
        call = RecordingEngine.__getattr__(self, name)

        def wrapped(*a, **k):
            got = call(*a, **k)
            if name == "set_polar":
                self._n_bins = a[1]
            if name == "polar_detect":
                return np.zeros((k["B"], a[1], self._n_bins))
            return got
        return wrapped


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", Engine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)


def test_constructor_refusals():
    from pyslice_amd import BandLimit, Detector
    from pyslice_amd.prism import Prism
    for kw in (dict(layers=[0]), dict(thickness=[0], detectors=_dets()), dict(prism=Prism(1)), dict(cache=True), dict(stream_tile=2),
               dict(tds=True, detectors=[Detector("haadf", inner=60.0, outer=200.0)])):
        for bl in (BandLimit(), 0.5):
            with pytest.raises(NotImplementedError, match="bandlimit: .* is not built"):
                _calc(bandlimit=bl, **kw)
        _calc(bandlimit=None, **kw)                                          # without a limit: accepted as ever
    with pytest.raises(ValueError, match="BandLimit"):
        _calc(bandlimit=0.7)
    with pytest.raises(ValueError, match="BandLimit"):
        _calc(bandlimit=0)
    with pytest.raises(ValueError, match="bandlimit"):
        _calc(bandlimit="2/3")


def test_several_ranks_are_refused_before_device_work(monkeypatch):
    from pyslice_amd import BandLimit, _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("device work before the check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    calc = _calc(bandlimit=BandLimit())
    with pytest.raises(NotImplementedError, match="bandlimit.*ranks is not built"):
        _setup(calc)
    assert calc._engine is None


def test_aperture_beyond_the_band_is_refused(recorder):
    from pyslice_amd import BandLimit
    calc = _setup(_calc(bandlimit=BandLimit()), aperture=0.0)                 # a plane wave is fine
    lim = calc.band_limit_mrad
    cx, cy = BandLimit().cuts(calc.nx, calc.ny, calc.dx, calc.dy)
    from pyslice_amd.multislice import wavelength
    assert lim == pytest.approx(1e3 * wavelength(100e3) * min(cx / (calc.nx * calc.dx), cy / (calc.ny * calc.dy)), rel=1e-14)
    _setup(_calc(bandlimit=BandLimit()), aperture=lim)                        # on the edge: the probe's own mask is strict
    with pytest.raises(ValueError, match="bandlimit.*aperture"):
        _setup(_calc(bandlimit=BandLimit()), aperture=lim * 1.01)
    assert _setup(_calc()).band_limit_mrad is None


def _modes():
    from pyslice_amd import Aberrations, Diffraction, PolarDetector
    return (dict(), dict(detectors=_dets()), dict(polar=PolarDetector(outer=40.0)), dict(diffraction=Diffraction()),
            dict(diffraction=Diffraction(split=True)), dict(k_window=(16, 16)), dict(k_bin=(2, 2)), dict(k_window=(16, 16), k_bin=(2, 4)),
            dict(aberrations=Aberrations(defocus=100.0, Cs=1e5)), dict(detectors=_dets(), aberrations=Aberrations(defocus=100.0)), dict(detectors=_dets(), probe_batch=2, frame_batch=2))


def _run(calc, kw):
    if "polar" in kw:
        return calc.run_polar()
    if "diffraction" in kw:
        return calc.run_diffraction()
    if "detectors" in kw:
        return calc.run_detectors()
    return calc.run()


def test_no_limit_issues_exactly_the_calls_of_a_run_without_the_argument(recorder):
    for kw in _modes():
        a = _setup(_calc(**kw)); _run(a, kw)
        b = _setup(_calc(bandlimit=None, **kw)); _run(b, kw)
        assert b._engine.created == a._engine.created
        assert format_calls(b._engine.calls, PP) == format_calls(a._engine.calls, PP), kw
        assert not [c for c in b._engine.calls if c[0] == "set_bandlimit"]


def test_the_limit_is_set_once_after_set_up_and_before_the_first_build(recorder):
    from pyslice_amd import BandLimit, Precession, Tilt
    from pyslice_amd.thermal import FrozenPhonons
    bl = BandLimit()
    builds = ("build_potential", "build_potentials", "build_thermal", "build_modes")
    for kw in _modes() + (dict(tilt=Tilt(10.0, 0.0)), dict(detectors=_dets(), precession=Precession(10.0, 3))):
        plain = _setup(_calc(**kw)); _run(plain, kw)
        calc = _setup(_calc(bandlimit=bl, **kw)); _run(calc, kw)
        names = [c[0] for c in calc._engine.calls]
        assert names.count("set_bandlimit") == 1, kw
        i = names.index("set_bandlimit")
        assert calc._engine.calls[i][1] == bl.cuts(calc.nx, calc.ny, calc.dx, calc.dy)
        assert names.index("set_slices") < i                                 # after the engine's set-up ..
        first_build = min(names.index(n) for n in builds if n in names)
        assert i < first_build, kw                                           # .. and before the first build
        # and nothing else changes: the calls without the one set_bandlimit are those of the plain run
        rest = [c for c in calc._engine.calls if c[0] != "set_bandlimit"]
        assert format_calls(rest, PP) == format_calls(plain._engine.calls, PP), kw
    tr = _trajectory(1)
    fp = FrozenPhonons(tr.atom_types, tr.positions[0], tr.box_matrix, sigma=0.05, n_configs=2, seed=1)
    calc = _calc(bandlimit=0.5)
    calc.setup(fp, aperture=20.0, voltage_eV=100e3, probe_positions=PP)
    calc.run()
    names = [c[0] for c in calc._engine.calls]
    assert names.count("set_bandlimit") == 1 and names.index("set_bandlimit") < names.index("build_thermal")
    assert calc._engine.calls[names.index("set_bandlimit")][1] == BandLimit(0.5).cuts(calc.nx, calc.ny, calc.dx, calc.dy)
    # the other two sources: phonon modes (generated like the configurations) and the absorptive potential, whose set_absorption
    # drops the potential and therefore comes with the limit before the first build too
    from pyslice_amd import AbsorptivePotential
    from pyslice_amd.phonons import PhononModes
    rng = np.random.default_rng(0)
    pm = PhononModes(tr.atom_types, tr.positions[0], tr.box_matrix, rng.integers(0, 2, tr.n_atoms), rng.random((3, 3)), rng.random(3),
                     rng.standard_normal((3, 2, 3)) * (0.02 + 0j), 2, seed=1)
    ab = AbsorptivePotential(tr.atom_types, tr.positions[0], tr.box_matrix, 0.05)
    for src, build in ((pm, "build_modes"), (ab, "build_potential")):
        for kw in (dict(), dict(detectors=_dets())):
            out = []
            for bl_kw in (dict(), dict(bandlimit=bl)):
                calc = _calc(**bl_kw, **kw)
                calc.setup(src, aperture=20.0, voltage_eV=100e3, probe_positions=PP)
                _run(calc, kw)
                out.append(calc._engine.calls)
            names = [c[0] for c in out[1]]
            assert names.count("set_bandlimit") == 1 and names.index("set_slices") < names.index("set_bandlimit") < names.index(build)
            assert format_calls([c for c in out[1] if c[0] != "set_bandlimit"], PP) == format_calls(out[0], PP)


def test_propagate_sets_and_clears_the_limit_of_the_shared_engine():
    from pyslice_amd import BandLimit, multislice

    class Eng(RecordingEngine):
        def __getattr__(self, name):
            call = RecordingEngine.__getattr__(self, name)

            def wrapped(*a, **k):
                call(*a, **k)
                if name == "get_tilt":
                    return (0.0, 0.0)
                if name == "exit_waves":
                    return np.zeros((1, self.wx, self.wy), dtype=np.complex64)
            return wrapped

    class Pot:
        xs = ys = np.arange(16) * 0.1
        zs = np.arange(3) * 2.0
        _engine = Eng(16, 16, 3)

    probe = multislice.Probe(Pot.xs, Pot.ys, 0.0, 100e3)
    multislice.Propagate(probe, Pot)
    multislice.Propagate(probe, Pot, bandlimit=None)
    assert not [c for c in Pot._engine.calls if "bandlimit" in c[0]]          # never limited: the engine is left alone
    multislice.Propagate(probe, Pot, bandlimit=BandLimit(0.5))
    multislice.Propagate(probe, Pot)                                         # the limit stays on the handle: it is taken off again
    multislice.Propagate(probe, Pot)
    assert [c[1] for c in Pot._engine.calls if c[0] == "set_bandlimit"] == [BandLimit(0.5).cuts(16, 16, 0.1, 0.1), (-1, -1)]
    n = len(Pot._engine.calls)
    multislice.Propagate(probe, Pot, bandlimit=BandLimit())
    multislice.Propagate(probe, Pot, bandlimit=2.0 / 3.0)                    # the cuts the engine carries already: no second call
    multislice.Propagate(probe, Pot, bandlimit=0.5)                          # other cuts: one call
    assert [c[1] for c in Pot._engine.calls[n:] if c[0] == "set_bandlimit"] == [BandLimit().cuts(16, 16, 0.1, 0.1),
                                                                                BandLimit(0.5).cuts(16, 16, 0.1, 0.1)]
    n = len(Pot._engine.calls)
    lim = BandLimit(0.5).max_angle_mrad(probe.wavelength, 16, 16, 0.1, 0.1)
    with pytest.raises(ValueError, match="bandlimit.*aperture"):              # refused before any call on the engine
        multislice.Propagate(multislice.Probe(Pot.xs, Pot.ys, 1.01 * lim, 100e3), Pot, bandlimit=0.5)
    assert len(Pot._engine.calls) == n
    multislice.Propagate(multislice.Probe(Pot.xs, Pot.ys, lim, 100e3), Pot, bandlimit=0.5)
    names = [c[0] for c in Pot._engine.calls]
    i = names.index("set_bandlimit")
    assert names.index("set_beam") < i < names.index("propagate", i)
    with pytest.raises(ValueError, match="bandlimit"):
        multislice.Propagate(probe, Pot, bandlimit="x")


# ------------------------------------------------------------------ 4. the ABI
def test_entry_points_in_the_header_and_binding():
    """The two calls are additions: the header keeps the version the binding checks at load (every feature since version 3 has
    added entry points without a bump, and the host tests of each pin the value)."""
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"int\s+msl_set_bandlimit\(msl_handle\* h, int32_t cut_x, int32_t cut_y\);", hdr)
    assert re.search(r"int\s+msl_get_bandlimit\(const msl_handle\* h, int32_t\* cut_xy\);", hdr)
    for name in ("msl_set_bandlimit", "msl_get_bandlimit"):
        assert name in _native.EXPORTS
    version = int(re.search(r"#define\s+MSL_ABI_VERSION\s+(\d+)\b", hdr).group(1))
    assert version == _native.ABI_VERSION


def test_the_library_exports_the_entry_points():
    from pyslice_amd import _native
    lib = _native.load()
    assert hasattr(lib, "msl_set_bandlimit") and hasattr(lib, "msl_get_bandlimit")
    assert lib.msl_set_bandlimit(None, 4, 4) == _native.MSL_ERR_INVALID       # null handle: refused before any device work
    assert lib.msl_get_bandlimit(None, None) == _native.MSL_ERR_INVALID


def test_kernels_are_in_their_headers():
    csrc = os.path.join(REPO, "pyslice_amd", "csrc")
    prop = open(os.path.join(csrc, "propagator.h")).read()
    assert re.search(r"__global__ void[^;{]*\bpropagator_bandlimit_kernel\(", prop)
    assert prop.index("propagator_tables_kernel(") < prop.index("propagator_bandlimit_kernel(") < prop.index("conv_lag_kernel(")
    bl = open(os.path.join(csrc, "bandlimit.h")).read()
    assert re.search(r"__global__ void[^;{]*\bbandlimit_mask_kernel\(", bl)
    main = open(os.path.join(csrc, "mslice.hip")).read()
    assert '#include "bandlimit.h"' in main and "bandlimit_lowpass" in main
