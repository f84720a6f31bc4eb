"""Band limit on the MI355X: the masked propagator tables and the low-passed transmission stacks (msl_set_bandlimit) against the
float64 definition (pyslice_amd/bandlimit.py: propagate_bandlimited), through the calculator and through the C ABI on one grid per
line-kernel class, in both loop modes.  2-3 slices and 1-4 probes throughout.

Bounds.  Exit waves and spectra: rel-L2 < WAVE_TOL = 1e-4, the project's wave contract (tests/test_gpu_parity.py).  Transmission
stack: 1e-5 relative per image, the white-potential contract with a chirp-z axis (96 and 80 points are both such axes).
Intensities: 2e-4.

What is NOT asserted: an exit spectrum that is exactly 0.0 outside the band.  The recursion ends on a transmission (the oracle's
last operation is t_{nz-1} psi, not a propagation), so the exit spectrum of the definition carries the product terms up to
|h| <= 2 c and their fold-back beyond n - 2 c; the comparison over the WHOLE spectrum holds the device to exactly that content.
What is zero by construction -- the spectrum of every limited transmission slice outside the band -- is asserted on the downloaded
stack (below 1e-6 of the peak: the slices are stored in float32 in real space)."""
import functools

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4
EV = 100e3
DZ, SAMPLING = 2.0, 0.1


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _trajectory(nx, ny, nz, n_frames=1, seed=0, density=0.05):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(nx, nz, n_frames, ny=ny, slice_thickness=DZ, density=density, seed=seed + nx + 7 * ny)


def _grid(tr):
    from oracle import multislice_oracle as orc
    xs, ys, zs, *_ = orc.grid_from_box(tr.box_matrix, sampling=SAMPLING, slice_thickness=DZ)
    return np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), np.asarray(zs, dtype=np.float64)


def _positions(xs, ys, P):
    lx, ly = len(xs) * (xs[1] - xs[0]), len(ys) * (ys[1] - ys[0])
    return [(0.31 * lx, 0.62 * ly), (0.77 * lx, 0.18 * ly), (0.5 * lx, 0.5 * ly), (0.12 * lx, 0.4 * ly)][:P]


def _transmission64(xs, ys, zs, positions, Z):
    """exp(i sigma V) (nz, nx, ny) complex128 of the oracle's potential"""
    from oracle import multislice_oracle as orc
    V = orc.potential(xs, ys, zs, positions, np.asarray(Z))
    return np.exp(1j * orc.interaction_sigma(EV) * np.moveaxis(V, 2, 0))


def _probes64(xs, ys, mrad, pp):
    from oracle import multislice_oracle as orc
    return orc.batched_probes(orc.probe_array(xs, ys, mrad, EV), xs, ys, pp)


def _spectra(exit_waves):
    return np.fft.fftshift(np.fft.fft2(exit_waves, axes=(-2, -1)), axes=(-2, -1))


# ------------------------------------------------------------------ 1. the calculator against the definition
def test_calculator_matches_the_definition():
    """64 x 48, 3 slices, 2 probes: MultisliceCalculator(bandlimit=BandLimit()) against propagate_bandlimited.  (Fails without the
    feature: the constructor has no such argument, and the unlimited run is 1e-2 away.)"""
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    tr = _trajectory(64, 48, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    assert (len(xs), len(ys), len(zs)) == (64, 48, 3)
    pp = _positions(xs, ys, 2)
    bl = BandLimit()
    calc = ps.MultisliceCalculator(device=0, progress=False, bandlimit=bl)
    calc.setup(tr, aperture=30.0, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
    got = npy(calc.run().wavefunction_data)[:, 0, :, :, 0]
    cuts = bl.cuts(64, 48, xs[1] - xs[0], ys[1] - ys[0])
    assert calc._engine.get_bandlimit() == cuts
    assert calc.band_limit_mrad == pytest.approx(bl.max_angle_mrad(orc.wavelength(EV), 64, 48, xs[1] - xs[0], ys[1] - ys[0]))
    t = _transmission64(xs, ys, zs, tr.positions[0], tr.atom_types)
    psi0 = _probes64(xs, ys, 30.0, pp)
    args = (xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0])
    want = _spectra(propagate_bandlimited(psi0, t, *args, cuts))
    plain = _spectra(propagate_bandlimited(psi0, t, *args, None))
    e, e_plain = rel_l2(got, want), rel_l2(got, plain)
    print(f"bandlimit calculator 64 x 48: rel-L2 {e:.3e} against the definition, {e_plain:.3e} against the unlimited recursion")
    assert e < WAVE_TOL
    assert e_plain > 10 * WAVE_TOL                                          # the limit does something at this sampling


def test_no_limit_is_bitwise_the_run_without_the_argument():
    import pyslice_amd as ps
    tr = _trajectory(64, 48, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    out = []
    for kw in (dict(), dict(bandlimit=None)):
        calc = ps.MultisliceCalculator(device=0, progress=False, **kw)
        calc.setup(tr, aperture=30.0, voltage_eV=EV, probe_positions=_positions(xs, ys, 2), slice_thickness=DZ, sampling=SAMPLING)
        out.append(npy(calc.run().wavefunction_data).copy())
        assert calc._engine.get_bandlimit() == (-1, -1)
    assert np.array_equal(out[0], out[1])


# ------------------------------------------------------------------ 2. every table consumer, through the C ABI
# grid, slices: one shape per line-kernel class of the first axis, the other axis short (600 x 501: the class on the second axis)
CLASSES = [(256, 64, 3, "rowT"), (512, 64, 3, "rowT2"), (135, 64, 3, "mixed A*B"), (972, 64, 3, "mixed 2*A*B"),
           (100, 64, 3, "convolution M=256"), (600, 501, 2, "convolution M=1024 on y"), (2048, 64, 2, "wave kernel")]
CLASS_IDS = [f"{nx}x{ny}" for nx, ny, _, _ in CLASSES]


def _engine(nx, ny, nz, P, dx=SAMPLING, dy=SAMPLING, **kw):
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    return _native.Engine(nx, ny, nz, dx, dy, DZ, wavelength(EV), interaction_sigma(EV), n_probes=P, **kw)


@functools.lru_cache(maxsize=None)
def white_case(nx, ny, nz, tilt_mrad=None):
    """white V and white probes (every bin carries weight) and the float64 exit waves of the definition, once per grid"""
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.tilt import Tilt
    rng = np.random.default_rng(nx * 7 + ny)
    V = (rng.random((nz, nx, ny)) * (2.0 / interaction_sigma(EV))).astype(np.float32)        # phases up to 2 rad, white
    psi0 = (rng.standard_normal((2, nx, ny)) + 1j * rng.standard_normal((2, nx, ny))).astype(np.complex64)
    cuts = BandLimit().cuts(nx, ny, SAMPLING, SAMPLING)
    t = np.exp(1j * interaction_sigma(EV) * V.astype(np.float64))
    tilt = None if tilt_mrad is None else Tilt(*tilt_mrad)
    want = propagate_bandlimited(psi0.astype(np.complex128), t, SAMPLING, SAMPLING, wavelength(EV), DZ, cuts, tilt=tilt)
    return V, psi0, cuts, want


def _white_run(nx, ny, nz, two_pass, monkeypatch, tilt_mrad=None):
    from pyslice_amd.tilt import Tilt
    V, psi0, cuts, want = white_case(nx, ny, nz, tilt_mrad)
    if two_pass:
        monkeypatch.setenv("MSL_DEBUG", "1")                                 # (the debug switches are read under MSL_DEBUG only)
        monkeypatch.setenv("MSL_SLICE_PATH", "2")
    eng = _engine(nx, ny, nz, 2)
    try:
        if tilt_mrad is not None:
            eng.set_tilt(*Tilt(*tilt_mrad).tangents)
        eng.set_bandlimit(*cuts)
        assert eng.get_bandlimit() == cuts
        eng.upload_probes(psi0)
        eng.upload_potential(V)
        eng.propagate()
        got = eng.exit_waves().copy()
    finally:
        eng.close()
    return got, want


@pytest.mark.parametrize("two_pass", [False, True], ids=["planned", "two-pass"])
@pytest.mark.parametrize("nx,ny,nz,kind", CLASSES, ids=CLASS_IDS)
def test_every_table_consumer(nx, ny, nz, kind, two_pass, monkeypatch):
    got, want = _white_run(nx, ny, nz, two_pass, monkeypatch)
    e = rel_l2(got, want)
    print(f"bandlimit {nx} x {ny} ({kind}, {'two-pass' if two_pass else 'planned loop'}): exit rel-L2 {e:.3e}, bound {WAVE_TOL:.0e}")
    assert e < WAVE_TOL


@pytest.mark.parametrize("two_pass", [False, True], ids=["planned", "two-pass"])
def test_with_tilt(two_pass, monkeypatch):
    """256 x 64 under Tilt(20, -10): the masked tilted table"""
    got, want = _white_run(256, 64, 3, two_pass, monkeypatch, tilt_mrad=(20.0, -10.0))
    e = rel_l2(got, want)
    print(f"bandlimit 256 x 64 with Tilt(20, -10) ({'two-pass' if two_pass else 'planned loop'}): exit rel-L2 {e:.3e}")
    assert e < WAVE_TOL
    _, untilted = white_case(256, 64, 3)[2:]
    assert rel_l2(want, untilted) > 0.1                                      # (the tilt is no no-op here)


def test_refused_cuts():
    from pyslice_amd import _native
    eng = _engine(64, 48, 2, 1)
    try:
        for bad in ((-1, 4), (4, -1), (0, 4), (4, 0), (22, 4), (4, 16)):      # 3 * 22 >= 64, 3 * 16 >= 48
            with pytest.raises(ValueError):
                eng.set_bandlimit(*bad)
            assert eng.get_bandlimit() == (-1, -1)
        eng.set_bandlimit(21, 15)
        assert eng.get_bandlimit() == (21, 15)
        eng.set_bandlimit(-1, -1)
        assert eng.get_bandlimit() == (-1, -1)
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. the transmission stack
def _check_stack(eng, cuts, label):
    from pyslice_amd.bandlimit import bandlimit_transmission, mask
    from pyslice_amd.multislice import interaction_sigma
    V = eng.potential().astype(np.float64)
    got = eng.transmission().astype(np.complex128)
    want = bandlimit_transmission(np.exp(1j * interaction_sigma(EV) * V), *cuts)
    out = ~mask(V.shape[1], V.shape[2], *cuts).astype(bool)
    for s in range(V.shape[0]):
        e = rel_l2(got[s], want[s])
        F = np.abs(np.fft.fft2(got[s]))
        leak = F[out].max() / F.max()
        print(f"bandlimit stack {label} slice {s}: rel-L2 {e:.3e} (bound 1e-5), out-of-band / peak {leak:.3e} (bound 1e-6)")
        assert e < 1e-5
        assert leak < 1e-6
    return got


def test_transmission_stack_in_both_layouts():
    """96 x 80 x 3 on a one-pass handle (slices of both parities, so natural and transposed ones): the downloaded stack is the
    low-pass of exp(i sigma V) of the downloaded V, also after the loop mode has flipped to the two-pass loop and back (a tilt along
    the convolution axis x, set and cleared) -- a stack limited twice would pass this, one limited in the wrong orientation or lost
    in the switch would not; and V stays the unlimited potential."""
    from pyslice_amd.bandlimit import BandLimit
    from pyslice_amd.potentials import loadKirkland, slice_edges
    tr = _trajectory(96, 80, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    assert (len(xs), len(ys), len(zs)) == (96, 80, 3)
    cuts = BandLimit().cuts(96, 80, SAMPLING, SAMPLING)
    Z = np.asarray(tr.atom_types, dtype=np.int32)
    plain = _engine(96, 80, 3, 1, keep_potential=True)
    eng = _engine(96, 80, 3, 1, keep_potential=True)
    try:
        for e in (plain, eng):
            e.set_kirkland(loadKirkland())
            e.set_slices(*slice_edges(zs))
        eng.set_bandlimit(*cuts)
        plain.build_potential(tr.positions[0], Z)
        eng.build_potential(tr.positions[0], Z)
        assert np.array_equal(eng.potential(), plain.potential())            # V is not limited
        first = _check_stack(eng, cuts, "96 x 80 built")
        assert rel_l2(first, plain.transmission()) > 1e-4                    # (the low-pass is no no-op on this potential)
        assert np.array_equal(eng.transmission(), first)                     # a download does not change the stack
        eng.set_tilt(0.01, 0.0)                                              # along x, a convolution axis: the two-pass loop
        tilted = _check_stack(eng, cuts, "96 x 80 under a tilt")
        eng.set_tilt(0.0, 0.0)                                               # and back
        back = _check_stack(eng, cuts, "96 x 80 tilt cleared")
        assert np.array_equal(tilted, first) and np.array_equal(back, first)  # carried over by transposes: copies, bit for bit
    finally:
        plain.close()
        eng.close()


# ------------------------------------------------------------------ 4. off is off
def test_off_is_off():
    from pyslice_amd.bandlimit import BandLimit
    from pyslice_amd.potentials import loadKirkland, slice_edges
    tr = _trajectory(64, 48, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    Z = np.asarray(tr.atom_types, dtype=np.int32)
    cuts = BandLimit().cuts(64, 48, SAMPLING, SAMPLING)
    eng = _engine(64, 48, 3, 2)
    try:
        eng.set_kirkland(loadKirkland())
        eng.set_slices(*slice_edges(zs))
        eng.set_probes(30.0, np.asarray(_positions(xs, ys, 2)))
        runs = []
        for c in (None, cuts, (-1, -1)):
            if c is not None:
                eng.set_bandlimit(*c)
                with pytest.raises(RuntimeError):                            # the stack belongs to the limit it was built under
                    eng.propagate()
            eng.build_potential(tr.positions[0], Z)
            eng.propagate()
            runs.append(eng.exit_waves().copy())
    finally:
        eng.close()
    assert np.array_equal(runs[0], runs[2])
    assert rel_l2(runs[1], runs[0]) > 10 * WAVE_TOL


# ------------------------------------------------------------------ 5. through the modes
@functools.lru_cache(maxsize=None)
def modes_case():
    """64 x 64 x 3, a 4-position scan, 2 frozen-phonon configurations: the spectra of the definition, (P, T, nx, ny)"""
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    from pyslice_amd.thermal import FrozenPhonons
    tr = _trajectory(64, 64, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    assert (len(xs), len(ys), len(zs)) == (64, 64, 3)
    fp = FrozenPhonons(tr.atom_types, tr.positions[0], tr.box_matrix, sigma=0.08, n_configs=2, seed=3)
    pp = _positions(xs, ys, 4)
    cuts = BandLimit().cuts(64, 64, xs[1] - xs[0], ys[1] - ys[0])
    psi0 = _probes64(xs, ys, 30.0, pp)
    W = np.empty((4, 2, 64, 64), dtype=np.complex128)
    calc = _calc(fp, pp)
    for c in range(2):
        pos = calc._engine.thermal_positions(fp.seed, c)                     # the configuration as the device generates it
        print(f"bandlimit modes: configuration {c}, max |device - thermal.py| {np.abs(pos - fp.configuration(c)).max():.3e} A")
        t = _transmission64(xs, ys, zs, pos, tr.atom_types)
        W[:, c] = _spectra(propagate_bandlimited(psi0, t, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0], cuts))
    incident = float((np.abs(psi0[0]) ** 2).sum())
    return fp, pp, W, incident


def _calc(fp, pp, **kw):
    import pyslice_amd as ps
    calc = ps.MultisliceCalculator(device=0, progress=False, bandlimit=ps.BandLimit(), **kw)
    calc.setup(fp, aperture=30.0, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
    return calc


def test_run_on_the_configurations_matches_the_definition():
    """run() on the two configurations, generated on the device and fed as host frames"""
    fp, pp, W, _ = modes_case()
    for name, src in (("FrozenPhonons", fp), ("to_trajectory()", fp.to_trajectory())):
        got = npy(_calc(src, pp).run().wavefunction_data)[..., 0]
        errs = [rel_l2(got[:, c], W[:, c]) for c in range(2)]
        print(f"bandlimit run() on {name}: rel-L2 per configuration {errs}")
        assert max(errs) < WAVE_TOL


def test_detectors_diffraction_and_polar_carry_the_limit():
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.polar_data import polar_bins, polar_signals
    fp, pp, W, _ = modes_case()
    lam = orc.wavelength(EV)
    I = np.abs(W) ** 2
    dets = [ps.Detector("bf", outer=25.0), ps.Detector("adf", inner=50.0, outer=110.0), ps.Detector("haadf", inner=110.0, outer=300.0)]

    calc = _calc(fp, pp, detectors=dets, probe_batch=3)
    kxs, kys = calc._k_axes()
    res = calc.run_detectors()
    for d, det in enumerate(dets):
        m = det.member(npy(kxs), npy(kys), lam)
        want = (I * m[None, None]).sum(axis=(2, 3))
        e = rel_l2(npy(res.signals)[..., d], want)
        print(f"bandlimit run_detectors {det.name}: rel-L2 {e:.3e}")
        assert e < 2e-4

    res = _calc(fp, pp, diffraction=ps.Diffraction(split=True)).run_diffraction()
    e_i, e_e = rel_l2(npy(res.intensity), I.mean(axis=1)), rel_l2(npy(res.elastic), np.abs(W.mean(axis=1)) ** 2)
    print(f"bandlimit run_diffraction(split=True): intensity rel-L2 {e_i:.3e}, elastic {e_e:.3e}")
    assert e_i < 2e-4 and e_e < 2e-4

    pol = ps.PolarDetector(outer=120.0, step=10.0, n_azimuthal=4)
    res = _calc(fp, pp, polar=pol, frame_batch=2).run_polar()
    bins = polar_bins(pol, npy(kxs), npy(kys), lam)
    want = polar_signals(W, bins, pol.n_bins).mean(axis=1).reshape(4, pol.n_rings, pol.n_azimuthal)
    e = rel_l2(npy(res.signals), want)
    print(f"bandlimit run_polar: rel-L2 {e:.3e}")
    assert e < 2e-4


def test_images_and_spectrum_images_run():
    """one run each: finite, and no more intensity than went in (|t| = 1 before the low-pass, and both masks only remove)"""
    import pyslice_amd as ps
    fp, pp, W, incident = modes_case()
    img = _calc(fp, pp, imaging=ps.Imaging()).run_images()
    tot = npy(img.intensity).sum(axis=(-2, -1)) / incident
    print(f"bandlimit run_images: total intensity / incident {tot.ravel()}")
    assert np.isfinite(npy(img.intensity)).all() and (tot <= 1 + 1e-5).all() and (tot > 0.5).all()
    res = _calc(fp, pp, spectroscopy=ps.Spectroscopy([ps.Detector("all", outer=1e4)])).run_spectrum_image()
    spec = npy(res.spectra)
    # Parseval along time and over the pixels: sum_f I <= T^2 nx ny incident
    tot = spec.sum(axis=(1, 2)) / (2 * 2 * 64 * 64 * incident)
    print(f"bandlimit run_spectrum_image: total intensity / bound {tot}")
    assert np.isfinite(spec).all() and (spec >= 0).all() and (tot <= 1 + 1e-5).all()


# ------------------------------------------------------------------ 6. the refusals, on a real engine
def test_refusals():
    import pyslice_amd as ps
    from pyslice_amd.prism import Prism
    bl = ps.BandLimit()
    for kw in (dict(layers=[0]), dict(thickness=[0], detectors=[ps.Detector("bf", outer=20.0)]), dict(prism=Prism(1)), dict(cache=True),
               dict(stream_tile=2), dict(tds=True, detectors=[ps.Detector("haadf", inner=60.0, outer=200.0)])):
        with pytest.raises(NotImplementedError, match="bandlimit"):
            ps.MultisliceCalculator(device=0, progress=False, bandlimit=bl, **kw)
    with pytest.raises(ValueError, match="BandLimit"):
        ps.MultisliceCalculator(device=0, progress=False, bandlimit=0.7)
    tr = _trajectory(64, 48, 3)
    calc = ps.MultisliceCalculator(device=0, progress=False, bandlimit=bl)
    with pytest.raises(ValueError, match="bandlimit.*aperture"):
        calc.setup(tr, aperture=150.0, voltage_eV=EV, slice_thickness=DZ, sampling=SAMPLING)
    calc.setup(tr, aperture=0.0, voltage_eV=EV, slice_thickness=DZ, sampling=SAMPLING)      # a plane wave is fine
    assert np.isfinite(npy(calc.run().wavefunction_data)).all()


# ------------------------------------------------------------------ 7. the other carried sources and options
def _check_transmission(eng, t_unlimited, cuts, label):
    """the downloaded stack against the low-pass of the float64 transmission functions, per image (1e-5: the stack contract)"""
    from pyslice_amd.bandlimit import bandlimit_transmission
    got = eng.transmission().astype(np.complex128)
    want = bandlimit_transmission(t_unlimited, *cuts)
    errs = [rel_l2(got[s], want[s]) for s in range(got.shape[0])]
    print(f"bandlimit stack {label}: rel-L2 per image {['%.3e' % e for e in errs]} (bound 1e-5)")
    assert max(errs) < 1e-5
    return got


def test_absorptive_potential_and_its_set_beam():
    """AbsorptivePotential at 64 x 64 x 3: the absorptive build (its own branch of the build) is limited -- run() against the
    definition fed t = exp(i sigma Vbar - sigma^2 Omega) of the two real stacks the engine keeps (unlimited, downloaded) -- and so is
    the stack msl_set_beam re-derives from them for another beam."""
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.absorptive import absorptive_transmission
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    tr = _trajectory(64, 64, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    ap = ps.AbsorptivePotential(tr.atom_types, tr.positions[0], tr.box_matrix, 0.08)
    pp = _positions(xs, ys, 2)
    calc = ps.MultisliceCalculator(device=0, progress=False, bandlimit=BandLimit())
    calc.setup(ap, aperture=30.0, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
    got = npy(calc.run().wavefunction_data)[:, 0, :, :, 0]
    eng = calc._engine
    cuts = eng.get_bandlimit()
    assert cuts == BandLimit().cuts(64, 64, xs[1] - xs[0], ys[1] - ys[0])
    Vbar, Om = eng.potential().astype(np.float64), eng.absorption().astype(np.float64)
    assert Om.max() > 0
    sig = orc.interaction_sigma(EV)
    t = absorptive_transmission(Vbar, Om, sig)
    _check_transmission(eng, t, cuts, "absorptive, built")
    want = _spectra(propagate_bandlimited(_probes64(xs, ys, 30.0, pp), t, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0], cuts))
    e = rel_l2(got, want)
    print(f"bandlimit AbsorptivePotential run(): rel-L2 {e:.3e}")
    assert e < WAVE_TOL
    # another beam: t again from the two stacks with the new sigma, limited again -- once, in the layout of the loop
    eV2 = 200e3
    eng.set_beam(orc.wavelength(eV2), orc.interaction_sigma(eV2), zs[1] - zs[0])
    t2 = absorptive_transmission(Vbar, Om, orc.interaction_sigma(eV2))
    again = _check_transmission(eng, t2, cuts, "absorptive, after set_beam")
    assert rel_l2(again, t2) > 1e-4                                          # (limited: not the unlimited stack)


def test_phonon_modes_carry_the_limit():
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    from pyslice_amd.phonons import PhononModes
    tr = _trajectory(64, 64, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    rng = np.random.default_rng(5)
    n, M, nb = len(tr.atom_types), 3, 2
    W = (rng.standard_normal((M, nb, 3)) + 1j * rng.standard_normal((M, nb, 3))) * 0.04
    pm = PhononModes(tr.atom_types, tr.positions[0], tr.box_matrix, rng.integers(0, nb, n), (rng.random((M, 3)) - 0.5) * 2.0, rng.random(M),
                     W, 2, seed=7)
    pp = _positions(xs, ys, 2)
    calc = ps.MultisliceCalculator(device=0, progress=False, bandlimit=BandLimit(), frame_batch=2)
    calc.setup(pm, aperture=30.0, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
    got = npy(calc.run().wavefunction_data)[..., 0]
    cuts = calc._engine.get_bandlimit()
    psi0 = _probes64(xs, ys, 30.0, pp)
    for c in range(2):
        t = _transmission64(xs, ys, zs, pm.configuration(c), tr.atom_types)
        want = _spectra(propagate_bandlimited(psi0, t, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0], cuts))
        e = rel_l2(got[:, c], want)
        print(f"bandlimit PhononModes frame {c}: rel-L2 {e:.3e}")
        assert e < WAVE_TOL
    assert rel_l2(got[:, 0], got[:, 1]) > 1e-3                               # (the frames are not one another)


def test_propagate_with_a_real_potential():
    """Propagate(probe, potential, bandlimit=): the rebuild of the stack from the kept V inside msl_set_bandlimit, which nothing else
    reaches (the potential is built before the limit is known) -- against the definition; the same cuts again make no call and give
    the same waves; bandlimit=None afterwards is bitwise a fresh unlimited Propagate."""
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    tr = _trajectory(64, 48, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    Z = np.asarray(tr.atom_types)

    def fresh():
        return ps.Potential(xs, ys, zs, tr.positions[0], Z, device=0), ps.Probe(xs, ys, 30.0, EV)
    pot, probe = fresh()
    plain = npy(ps.Propagate(probe, pot))
    bl = BandLimit()
    cuts = bl.cuts(64, 48, xs[1] - xs[0], ys[1] - ys[0])
    got = npy(ps.Propagate(probe, pot, bandlimit=bl))
    assert pot._engine.get_bandlimit() == cuts
    t = _transmission64(xs, ys, zs, tr.positions[0], Z)
    psi0 = orc.probe_array(xs, ys, 30.0, EV)
    want = propagate_bandlimited(psi0, t, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0], cuts)[0]
    e = rel_l2(got, want)
    print(f"bandlimit Propagate 64 x 48: rel-L2 {e:.3e} against the definition, {rel_l2(got, plain):.3e} against the unlimited call")
    assert e < WAVE_TOL and rel_l2(got, plain) > 10 * WAVE_TOL
    _check_transmission(pot._engine, t, cuts, "Propagate, rebuilt from the kept V")
    assert np.array_equal(npy(ps.Propagate(probe, pot, bandlimit=0.0 + bl.fraction)), got)     # the same cuts: the same stack
    off = npy(ps.Propagate(probe, pot))                                      # the limit comes off the shared engine again
    assert pot._engine.get_bandlimit() == (-1, -1)
    pot2, probe2 = fresh()
    assert np.array_equal(off, npy(ps.Propagate(probe2, pot2))) and np.array_equal(off, plain)
    with pytest.raises(ValueError, match="bandlimit.*aperture"):
        ps.Propagate(ps.Probe(xs, ys, 150.0, EV), pot, bandlimit=bl)


def test_aberrations_k_window_and_k_bin_carry_the_limit():
    """an aberrated probe (the device's own probes are the psi0 of the definition) and the stored window and bin of run(): the
    same NumPy reductions on the spectra of the definition"""
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.bandlimit import BandLimit, propagate_bandlimited
    tr = _trajectory(64, 64, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    pp = _positions(xs, ys, 2)
    t = _transmission64(xs, ys, zs, tr.positions[0], tr.atom_types)
    args = (xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0])
    cuts = BandLimit().cuts(64, 64, xs[1] - xs[0], ys[1] - ys[0])

    def run(**kw):
        calc = ps.MultisliceCalculator(device=0, progress=False, bandlimit=BandLimit(), **kw)
        calc.setup(tr, aperture=30.0, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
        got = npy(calc.run().wavefunction_data)[:, 0, :, :, 0]
        return got, calc._engine.probes().astype(np.complex128)

    flat = _spectra(propagate_bandlimited(_probes64(xs, ys, 30.0, pp), t, *args, cuts))
    got, psi0 = run(aberrations=ps.Aberrations(defocus=150.0, Cs=2.0e5, astigmatism=40.0, astigmatism_angle=0.4))
    want = _spectra(propagate_bandlimited(psi0, t, *args, cuts))
    e = rel_l2(got, want)
    print(f"bandlimit with aberrations: rel-L2 {e:.3e} (against the unaberrated run {rel_l2(got, flat):.3e})")
    assert e < WAVE_TOL and rel_l2(got, flat) > 0.1

    got, _ = run(k_window=(32, 48))
    want = flat[:, 32 - 16:32 + 16, 32 - 24:32 + 24]
    e = rel_l2(got, want)
    print(f"bandlimit with k_window=(32, 48): rel-L2 {e:.3e}")
    assert got.shape == want.shape and e < WAVE_TOL

    got, _ = run(k_window=(32, 48), k_bin=(2, 4))
    want = want.reshape(2, 16, 2, 12, 4).sum(axis=(2, 4))
    e = rel_l2(got, want)
    print(f"bandlimit with k_window=(32, 48), k_bin=(2, 4): rel-L2 {e:.3e}")
    assert got.shape == want.shape and e < WAVE_TOL
