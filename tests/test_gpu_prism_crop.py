"""PRISM probes synthesised on the cropped window grid (msl_smatrix_probes_cropped, Prism(f, crop=True)) on the device.  The cropped
spectrum is the full-grid spectrum of msl_smatrix_probes at every (fx, fy)-th pixel (prism.crop_index), so the existing path is
the reference; the float64 definition prism.prism_waves_cropped on the downloaded S-matrix is the second one.  Bounds are the
project's contracts: 1e-4 rel-L2 for waves and spectra, 2e-4 for intensities.
Cells: a few dozen gold atoms of pyslice_amd.synthetic, 4 slices of 0.5 A, 100 kV, 0.1 A pixels; the potential is the oracle's."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

EV = 100e3
WAVE_TOL = 1e-4
INTENSITY_TOL = 2e-4
D = 0.1
NZ = 4
MRAD = 30.0
# 64 x 64 / (2, 2): 16-byte path; 96 x 80 / (2, 4): unequal interpolations, 16-byte path; 90 x 70 / (2, 2): an odd 45 x 35 cropped
# grid, the 8-byte path.  5 probes: a ragged group of the G = 8 kernel; 11: the G = 16 kernel
GRIDS = [(64, 64, (2, 2)), (96, 80, (2, 4)), (90, 70, (2, 2))]
COUNTS = [5, 11]


def npy(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def spectrum(psi):
    return np.fft.fftshift(np.fft.fft2(psi, axes=(-2, -1)), axes=(-2, -1))


def positions(nx, ny, n):
    """the window of the first position wraps the cell edge on both axes (the probe peaks at pixel (0, 1)), the second lies half a
    pixel off the grid on both, the third wraps along x only; the rest are scattered"""
    rng = np.random.default_rng(nx * 1000 + ny)
    fixed = [(nx * D / 2, ny * D / 2 - D), (1.25, 0.35), (nx * D / 2 + 0.3, 0.7)]
    rest = rng.uniform(0.0, 1.0, (n - len(fixed), 2)) * [nx * D, ny * D]
    return np.ascontiguousarray(np.concatenate([np.array(fixed), rest]))


@functools.lru_cache(maxsize=None)
def potential(nx, ny):
    """(NZ, nx, ny) float32: the oracle's potential of a synthetic gold cell of a few dozen atoms"""
    from oracle import multislice_oracle as o
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, NZ, 1, ny=ny, density=0.3, seed=nx + ny, species=(79,))
    assert 20 <= len(tr.atom_types) <= 60
    xs, ys, zs = np.arange(nx) * D, np.arange(ny) * D, np.arange(NZ) * 0.5
    V = o.potential(xs, ys, zs, tr.positions[0], tr.atom_types)
    return np.ascontiguousarray(np.moveaxis(V, 2, 0)).astype(np.float32)


def engine(nx, ny, nz, P, n_frames, with_potential=False, dx=D, lam=None, **kw):
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    eng = _native.Engine(nx, ny, nz, dx, dx, 0.5, wavelength(EV) if lam is None else lam, interaction_sigma(EV), n_probes=P,
                         n_frames=n_frames, **kw)
    if with_potential:
        eng.upload_potential(potential(nx, ny))
    return eng


def _aberrations():
    from pyslice_amd.aberrations import Aberrations
    return Aberrations(defocus=150.0, Cs=2e5, astigmatism=40.0, astigmatism_angle=0.7)


@functools.lru_cache(maxsize=None)
def case(nx, ny, f, P, aberrated=False, window=None):
    """One device run per configuration, shared by the tests: the full-grid spectra of msl_smatrix_probes (slot 0 of the source),
    the cropped spectra of two identical calls (slots 1 and 0 of the result handle), the folded exit waves, S and its beams"""
    xy = positions(nx, ny, P)
    src = engine(nx, ny, NZ, P, 1, with_potential=True)
    dst = engine(nx // f[0], ny // f[1], 1, P, 2, window=window)         # no potential, one slice
    try:
        src.smatrix_begin(f, MRAD)
        src.smatrix_build()
        src.set_aberrations(_aberrations() if aberrated else None)
        src.smatrix_probes(xy, 0)
        full = src.frame(0)
        src.smatrix_probes_cropped(dst, xy, 1)
        first, exit_c = dst.frame(1), dst.exit_waves()
        src.smatrix_probes_cropped(dst, xy, 0)
        again, exit_again = dst.frame(0), dst.exit_waves()
        out = dict(xy=xy, full=full, crop=first, again=again, exit=exit_c, exit_again=exit_again, S=src.smatrix(), hb=src.smatrix_beams())
    finally:
        dst.close()
        src.close()
    for v in out.values():
        v.setflags(write=False)
    return out


def _definition(c, f, aberrated=False):
    from pyslice_amd import prism
    from pyslice_amd.multislice import wavelength
    return prism.prism_waves_cropped(c["S"].astype(np.complex128), c["hb"], c["xy"], D, D, f, wavelength(EV),
                                     _aberrations() if aberrated else None)


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("nx,ny,f", GRIDS)
def test_cropped_slot_is_the_full_slot_at_crop_index(nx, ny, f, P):
    from pyslice_amd import prism
    c = case(nx, ny, f, P)
    ix, iy = prism.crop_index(nx, f[0]), prism.crop_index(ny, f[1])
    want = c["full"][:, ix[:, None], iy[None, :]]
    assert c["crop"].shape == want.shape == (P, nx // f[0], ny // f[1])
    errs = [rel_l2(c["crop"][p], want[p]) for p in range(P)]
    print(f"{nx} x {ny} f = {f} P = {P}: cropped slot against the full slot at crop_index, worst rel-L2 {max(errs):.3e}")
    assert max(errs) < WAVE_TOL


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("nx,ny,f", GRIDS)
def test_cropped_slot_and_exit_against_the_float64_definition(nx, ny, f, P):
    c = case(nx, ny, f, P)
    want = _definition(c, f)
    e_exit = [rel_l2(c["exit"][p], want[p]) for p in range(P)]
    e_spec = [rel_l2(c["crop"][p], spectrum(want[p])) for p in range(P)]
    print(f"{nx} x {ny} f = {f} P = {P}: against the folded definition, exit {max(e_exit):.3e} spectrum {max(e_spec):.3e}")
    assert max(e_exit) < WAVE_TOL and max(e_spec) < WAVE_TOL
    assert np.abs(c["exit"]).min() > 0                                   # every cropped pixel was written: no hole, no zero fill


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("nx,ny,f", GRIDS)
def test_two_calls_are_bitwise_equal(nx, ny, f, P):
    c = case(nx, ny, f, P)
    assert np.array_equal(c["crop"].view(np.uint32), c["again"].view(np.uint32))
    assert np.array_equal(c["exit"].view(np.uint32), c["exit_again"].view(np.uint32))


def test_aberrations_are_the_source_handles():
    from pyslice_amd import prism
    nx, ny, f, P = 96, 80, (2, 4), 5
    c, plain = case(nx, ny, f, P, aberrated=True), case(nx, ny, f, P)
    ix, iy = prism.crop_index(nx, f[0]), prism.crop_index(ny, f[1])
    want = _definition(c, f, aberrated=True)
    for p in range(P):
        e = (rel_l2(c["crop"][p], c["full"][p][ix[:, None], iy[None, :]]), rel_l2(c["crop"][p], spectrum(want[p])), rel_l2(c["exit"][p], want[p]))
        print(f"aberrated, probe {p}: slot against full {e[0]:.2e}, against the definition {e[1]:.2e}, exit {e[2]:.2e}")
        assert max(e) < WAVE_TOL
        assert rel_l2(c["crop"][p], plain["crop"][p]) > 100 * WAVE_TOL   # and the aberrations did something


def test_k_window_on_the_result_handle():
    """the result handle's k-window is centred on the cropped DC pixel: an even and an odd window of the odd 45 x 35 grid too"""
    from pyslice_amd import prism
    for nx, ny, f, window in ((64, 64, (2, 2), (16, 24)), (90, 70, (2, 2), (21, 16))):
        c = case(nx, ny, f, 5, window=window)
        wx, wy = nx // f[0], ny // f[1]
        x0, y0 = wx // 2 - window[0] // 2, wy // 2 - window[1] // 2
        ix, iy = prism.crop_index(nx, f[0])[x0:x0 + window[0]], prism.crop_index(ny, f[1])[y0:y0 + window[1]]
        want = c["full"][:, ix[:, None], iy[None, :]]
        assert c["crop"].shape == want.shape == (5,) + window
        errs = [rel_l2(c["crop"][p], want[p]) for p in range(5)]
        print(f"{nx} x {ny} f = {f} k-window {window}: worst rel-L2 {max(errs):.3e}")
        assert max(errs) < WAVE_TOL
        assert np.array_equal(c["crop"].view(np.uint32), c["again"].view(np.uint32))


def test_source_without_a_result_and_with_another_probe_count():
    """the source's n_probes is only the chunk of the build, and it needs no result ring: 3 against 5 probes, n_frames = 0"""
    nx, ny, f, P = 64, 64, (2, 2), 5
    c = case(nx, ny, f, P)
    src = engine(nx, ny, NZ, 3, 0, with_potential=True)
    dst = engine(nx // 2, ny // 2, 1, P, 1)
    try:
        src.smatrix_begin(f, MRAD)
        src.smatrix_build()
        src.smatrix_probes_cropped(dst, c["xy"], 0)
        got, wave = dst.frame(0), dst.exit_waves()
    finally:
        dst.close()
        src.close()
    # the chunk changes neither S (each beam's slice loop is its own) nor the synthesis
    assert np.array_equal(got.view(np.uint32), c["crop"].view(np.uint32)) and np.array_equal(wave.view(np.uint32), c["exit"].view(np.uint32))


def test_every_error_return():
    """argument checks only: nothing is launched by a refused call"""
    import torch
    from pyslice_amd import _native
    from pyslice_amd.multislice import wavelength
    lib = _native.load()
    nx, ny, f, P = 64, 64, (2, 2), 3
    xy = positions(nx, ny, P)
    bad_xy = [xy.copy(), xy.copy()]
    bad_xy[0][1, 0] = np.nan
    bad_xy[1][2, 1] = np.inf

    def rc(src, dst, pts, n, slot):
        return lib.msl_smatrix_probes_cropped(src._h if src is not None else None, dst._h if dst is not None else None,
                                              pts.ctypes.data_as(ctypes.c_void_p) if pts is not None else None, n, slot)
    INVALID, STATE = _native.MSL_ERR_INVALID, _native.MSL_ERR_STATE
    src = engine(nx, ny, 2, 2, 0)
    others = dict(good=engine(32, 32, 1, P, 2), grid=engine(32, 16, 1, P, 2), full=engine(64, 64, 1, P, 2), pixel=engine(32, 32, 1, P, 2, dx=0.15),
                  lam=engine(32, 32, 1, P, 2, lam=wavelength(80e3)), count=engine(32, 32, 1, P + 1, 2), ringless=engine(32, 32, 1, P, 0))
    if torch.cuda.device_count() > 1:
        others["device"] = engine(32, 32, 1, P, 2, device=1)
    try:
        good = others["good"]
        assert rc(src, good, xy, P, 0) == STATE                          # before begin
        src.smatrix_begin(f, MRAD)
        assert rc(src, good, xy, P, 0) == STATE                          # begun, not built
        src.upload_potential(np.zeros((2, nx, ny), dtype=np.float32))
        src.smatrix_build()
        assert rc(None, good, xy, P, 0) == INVALID and rc(src, None, xy, P, 0) == INVALID and rc(src, good, None, P, 0) == INVALID
        assert rc(src, src, xy, 2, 0) == INVALID                         # a handle is not its own cropped grid
        for name in ("grid", "full", "pixel", "lam", "count"):
            assert rc(src, others[name], xy, P, 0) == INVALID, name
        if "device" in others:
            assert rc(src, others["device"], xy, P, 0) == INVALID
        else:
            print("one device visible: the different-devices refusal was not exercised")
        assert rc(src, good, xy, P - 1, 0) == INVALID and rc(src, good, xy, P + 1, 0) == INVALID
        assert rc(src, good, xy, P, -1) == INVALID and rc(src, good, xy, P, 2) == INVALID
        assert rc(src, good, bad_xy[0], P, 0) == INVALID and rc(src, good, bad_xy[1], P, 0) == INVALID
        assert rc(src, others["ringless"], xy, P, 0) == STATE
        with pytest.raises(ValueError, match="msl_smatrix_probes_cropped"):
            src.smatrix_probes_cropped(others["grid"], xy, 0)            # the binding raises with the library's message
        with pytest.raises(RuntimeError, match="n_frames == 0"):
            src.smatrix_probes_cropped(others["ringless"], xy, 0)
        assert not np.asarray(good.frame(0)).any() and not np.asarray(good.frame(1)).any()    # no refused call wrote anything
        assert rc(src, good, xy, P, 1) == _native.MSL_OK                 # and the accepted one does
        assert np.asarray(good.frame(1)).any() and not np.asarray(good.frame(0)).any()
    finally:
        for e in others.values():
            e.close()
        src.close()


# ---- the calculator: 64 x 64, Prism(2, crop=True) against Prism(2), 2 frames, 9 probes in batches of 4 ------------------------
@functools.lru_cache(maxsize=None)
def scan():
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 6, 2, density=0.2, seed=5, species=(79,))
    assert 20 <= len(tr.atom_types) <= 60
    pp = [(3.2, 3.1), (1.25, 0.35), (3.5, 0.7)] + [tuple(v) for v in np.random.default_rng(6).random((6, 2)) * 6.4]
    return tr, pp


def _detectors():
    import pyslice_amd as ps
    return [ps.Detector("bf", outer=30.0), ps.Detector("adf", inner=40.0, outer=120.0), ps.Detector("half", outer=60.0, azimuth=(0.0, 180.0))]


def _polar():
    import pyslice_amd as ps
    return ps.PolarDetector(outer=90.0, step=10.0, n_azimuthal=4, per_frame=True)


@functools.lru_cache(maxsize=None)
def run(mode, crop, source="md"):
    """one calculator run per (mode, crop, source), shared: -> the result object"""
    import pyslice_amd as ps
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.prism import Prism
    tr, pp = scan()
    if source == "phonons":
        tr = ps.FrozenPhonons(tr.atom_types, tr.positions[0], tr.box_matrix, 0.05, n_configs=2, seed=3)
    kw = dict(run=dict(dtype="complex64"), run_diffraction=dict(diffraction=Diffraction(bin=(1, 1)), probe_batch=4),
              run_detectors=dict(detectors=_detectors(), probe_batch=4), run_polar=dict(polar=_polar(), detectors=_detectors(), probe_batch=4))[mode]
    calc = ps.MultisliceCalculator(device=0, progress=False, prism=Prism(2, crop=crop), **kw)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    if crop:
        beam, res = calc._beam_engine, calc._engine
        assert (beam.nx, beam.ny, beam.n_frames) == (64, 64, 0) and (res.nx, res.ny, res.nz) == (32, 32, 1)
        assert beam.n_probes == min(res.n_probes, calc._prism_Bm)
        assert mode == "run" or (calc.probe_batch == res.n_probes == 4 and res.n_frames == 1)
    out = getattr(calc, mode)()
    assert getattr(out, "prism_crop", None) == ((2, 2) if crop else None)
    return out


def _idx():
    from pyslice_amd import prism
    i = prism.crop_index(64, 2)
    return i[:, None], i[None, :]


def test_run_diffraction_patterns_are_the_uncropped_ones_at_crop_index():
    got, ref = run("run_diffraction", True), run("run_diffraction", False)
    ix, iy = _idx()
    a, b = npy(got.intensity), npy(ref.intensity)[:, ix, iy]
    assert a.shape == b.shape == (9, 32, 32)
    errs = [rel_l2(a[p], b[p]) for p in range(9)]
    print(f"run_diffraction, Prism(2, crop=True) against Prism(2) at crop_index: worst rel-L2 {max(errs):.3e}")
    assert max(errs) < INTENSITY_TOL
    assert np.allclose(npy(got.kxs), npy(ref.kxs)[ix[:, 0]], rtol=1e-6, atol=0) and np.allclose(npy(got.kys), npy(ref.kys)[iy[0]], rtol=1e-6, atol=0)
    # not rescaled: each cropped pixel stands for fx fy full ones
    ratio = npy(ref.intensity).sum(axis=(1, 2)) / a.sum(axis=(1, 2))
    print(f"sum of the uncropped pattern / sum of the cropped one: {ratio.min():.4f} .. {ratio.max():.4f}")
    assert np.allclose(ratio, 4.0, rtol=1e-3)


def test_run_spectra_are_the_uncropped_ones_at_crop_index():
    got, ref = run("run", True), run("run", False)
    ix, iy = _idx()
    a, b = npy(got.wavefunction_data)[..., 0], npy(ref.wavefunction_data)[..., 0][:, :, ix, iy]
    assert a.shape == b.shape == (9, 2, 32, 32)
    errs = [rel_l2(a[p, t], b[p, t]) for p in range(9) for t in range(2)]
    print(f"run(), Prism(2, crop=True) against Prism(2) at crop_index: worst rel-L2 {max(errs):.3e}")
    assert max(errs) < WAVE_TOL
    assert len(got.kxs) == 32 and len(got.kys) == 32


def _host_detector_sums(patterns, kx, ky):
    """(P, D): the detectors' masks summed on the host over the patterns (P, mx, my), and the same of the moduli"""
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.stem_data import detector_bitmask
    dets = _detectors()
    bits = detector_bitmask(dets, kx, ky, wavelength(EV))
    masks = [((bits >> d) & 1).astype(bool) for d in range(len(dets))]
    assert all(m.any() for m in masks)
    return np.stack([patterns[:, m].sum(axis=1) for m in masks], axis=1)


@pytest.mark.parametrize("source", ["md", "phonons"])
def test_run_detectors_are_the_masks_over_the_cropped_patterns(source):
    """signals (P, T, D) averaged over the frames against the masks summed over the frame-averaged cropped patterns; the addends are
    non-negative, so the bound of test_gpu_detectors' host sums (1e-6 of the sum of the moduli) is 1e-6 of the value"""
    st, dd = run("run_detectors", True, source), run("run_diffraction", True, source)
    sig = npy(st.signals)
    assert sig.shape == (9, 2, 3) and len(st.kxs) == 32
    want = _host_detector_sums(npy(dd.intensity), npy(st.kxs), npy(st.kys))
    err = np.abs(sig.mean(axis=1) - want) / want
    print(f"run_detectors ({source}) against the host sums over run_diffraction's cropped patterns: worst {err.max():.3e}")
    assert err.max() <= 1e-6
    if source == "phonons":
        assert rel_l2(sig[:, 0], sig[:, 1]) > 1e-3                       # two different configurations


def test_run_polar_bins_are_the_bins_over_the_cropped_patterns():
    import pyslice_amd as ps
    from pyslice_amd.multislice import wavelength
    res, dd = run("run_polar", True), run("run_diffraction", True)
    req = _polar()
    sig = npy(res.signals)
    assert sig.shape == (9, 2, req.n_rings, req.n_azimuthal) and len(res.kxs) == 32
    bins = np.asarray(ps.polar_bins(req, npy(res.kxs), npy(res.kys), wavelength(EV))).reshape(-1)
    pat = npy(dd.intensity).reshape(9, -1)
    keep = bins != 0xFFFF                                                # (POLAR_NONE: a pixel in no bin)
    want = np.stack([np.bincount(bins[keep].astype(np.int64), weights=pat[p][keep], minlength=req.n_bins) for p in range(9)])
    got = sig.mean(axis=1).reshape(9, -1)
    filled = want > 0
    err = np.abs(got[filled] - want[filled]) / want[filled]
    print(f"run_polar against the host bins over run_diffraction's cropped patterns: worst {err.max():.3e}")
    assert err.max() <= 1e-6 and not got[~filled].any()
    # detectors in the same pass: what run_detectors() gives alone
    assert np.array_equal(npy(res.stem.signals), npy(run("run_detectors", True).signals))
