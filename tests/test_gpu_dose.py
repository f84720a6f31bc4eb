"""Finite dose on the MI355X: the device's Poisson draws against the definition (pyslice_amd/dose.py), the accumulator against
run_diffraction() without a dose, reproducibility over seeds and probe batches, counting statistics, and the library's error codes.

Cells: 48 x 40 and 32 x 32 pixels of 0.1 A, 5 slices, 3 frames at a frame batch of 2, up to 5 probes at a probe batch of 2 (the last
batch is padded); k-windows with an odd row length take the 8-byte load path of the pattern pass."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EV, MRAD, T = 100e3, 30.0, 3


def _differing_allowed(n):
    return max(1, int(1e-4 * n))


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def _cell(ps, nx, ny, seed, P=5):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, 5, T, ny=ny, density=0.1, seed=seed)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(seed + 1).random((P, 2)) * [lx, ly]]
    return tr, pp


def _run(ps, tr, pp, dose=None, bin=(1, 1), probe_batch=2, frame_batch=2, k_window=None, detectors=None):
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=bin, dose=dose), probe_batch=probe_batch,
                                   frame_batch=frame_batch, k_window=k_window, detectors=detectors)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    assert calc.probe_batch == min(probe_batch, len(pp)) and calc._engine.frame_batch == frame_batch
    dd = calc.run_diffraction()
    dd.pixel = (calc.dx, calc.dy)
    return dd


def _expected(dd):
    """lam of every pixel as the host forms it from the returned float64 mean: intensity * T * scale"""
    scale = dd.electrons_per_probe / (dd.n_frames * dd.incident)
    return dd.intensity * dd.n_frames * scale


N_E, SEED = 2.0e4, 5


@pytest.fixture(scope="module")
def base(ps):
    """the run most tests share: 48 x 40, 5 probes in batches of 2, 3 frames in batches of 2, intensity kept"""
    tr, pp = _cell(ps, 48, 40, 31)
    dd = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED, keep_intensity=True))
    return tr, pp, dd


# ------------------------------------------------------------------ 1. the sampler
def test_counts_match_the_definition(ps, base):
    """the device's counts are poisson_counts() of the float64 it returns, pixel for pixel: the disc draws by PTRS, the tails by
    inversion.  Licensed: a last-place difference of exp / log / lgamma that flips a comparison, about 1e-13 per pixel"""
    tr, pp, dd = base
    assert dd.counts.shape == (5, 48, 40) and dd.counts.dtype == np.uint32 and dd.intensity.shape == (5, 48, 40)
    assert dd.electrons_per_probe == N_E and dd.dose.seed == SEED and dd.incident > 20
    lam = _expected(dd)
    n_ptrs, n_inv = int((lam >= 10).sum()), int(((lam > 0) & (lam < 1)).sum())
    print(f"lam in [{lam.min():.3e}, {lam.max():.3e}]: {n_ptrs} pixels on PTRS, {n_inv} below 1")
    assert n_ptrs >= 10 and n_inv >= 100
    want = ps.poisson_counts(lam, SEED, np.arange(5))
    differ = int((want != dd.counts).sum())
    print(f"{differ} of {lam.size} pixels differ")
    assert differ <= _differing_allowed(lam.size)


@pytest.mark.parametrize("shape,ld_pad,bin", [((45, 63), 0, (1, 1)), ((45, 63), 3, (5, 9)), ((32, 32), 0, (1, 4)), ((32, 32), 5, (2, 2)),
                                              ((48, 40), 0, (3, 5))])
def test_library_accumulates_and_draws_on_caller_memory(ps, shape, ld_pad, bin):
    """msl_dose_add in two calls is msl_diffract's two results added in float64, bit for bit, in every bin mode and on the 8-byte
    load path; msl_dose_counts of it is the definition over lam from 1e-6 to 1e7 and with probe0 > 0"""
    import torch
    from pyslice_amd import _native
    rng = np.random.default_rng(shape[0] + ld_pad)
    B, Tn, (wx, wy) = 3, 5, shape
    K, ld = wx * wy, wx * wy + ld_pad
    W = (rng.standard_normal((B, Tn, K)) + 1j * rng.standard_normal((B, Tn, K))).astype(np.complex64)
    # the amplitude grows with the row of bins, from 10^-3.5 to 10^3: the pixels of a bin share it, so lam spans 13 decades
    rows = np.repeat(np.linspace(-3.5, 3.0, wx // bin[0]), bin[0])
    W *= np.repeat(10.0 ** rows, wy).astype(np.float32)[None, None, :]
    host = np.zeros((B, Tn, ld), dtype=np.complex64)
    host[:, :, :K] = W
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    eng = _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        src = (dW.data_ptr(), B, Tn, wx, wy, ld)
        mx, my = wx // bin[0], wy // bin[1]
        want = eng.diffract(0, 2, bin=bin, src=src) + eng.diffract(2, 3, bin=bin, src=src)
        eng.dose_reset(B + 1, (mx, my))                                 # (sized for more probes than are added)
        eng.dose_add(0, 2, bin=bin, src=src)
        eng.dose_add(2, 3, bin=bin, src=src)
        counts, acc = eng.dose_counts(0.7, 77, probe0=1000, B=B, keep_intensity=True)
        assert acc.shape == (B, mx, my) and np.array_equal(acc, want)
        lam = acc * 0.7
        assert lam.min() < 1e-3 and lam.max() > 1e5
        ref = ps.poisson_counts(lam, 77, 1000 + np.arange(B))
        differ = int((ref != counts).sum())
        print(f"shape {shape} ld+{ld_pad} bin {bin}: lam in [{lam.min():.2e}, {lam.max():.2e}], {differ} of {lam.size} pixels differ")
        assert differ <= _differing_allowed(lam.size)
        again, none = eng.dose_counts(0.7, 77, probe0=1000, B=B)
        assert none is None and np.array_equal(again, counts)
        assert np.array_equal(eng.diffract(0, 2, bin=bin, src=src) + eng.diffract(2, 3, bin=bin, src=src), want)   # msl_diffract as it was
        eng.dose_reset(B, (mx, my))                                     # a reset starts a new sum
        eng.dose_add(0, 1, bin=bin, src=src)
        assert np.array_equal(eng.dose_counts(1.0, 1, B=B, keep_intensity=True)[1], eng.diffract(0, 1, bin=bin, src=src))
        assert not eng.dose_counts(0.0, 1, B=B)[0].any()                # scale 0: lam = 0, nothing drawn
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the accumulator
@pytest.mark.parametrize("grid,k_window,bin", [((48, 40), None, (1, 1)), ((48, 40), None, (2, 4)), ((48, 40), None, (3, 5)),
                                               ((32, 32), (15, 15), (1, 1)), ((32, 32), (15, 15), (3, 5))])
def test_intensity_is_that_of_a_run_without_dose(ps, grid, k_window, bin):
    """direct stores, the shuffle and the LDS bin mode, 16-byte and (odd rows of the k-window) 8-byte loads; the tolerance is the
    one test_gpu_diffraction.py holds frame splits to: 1e-6 of the pattern's maximum"""
    tr, pp = _cell(ps, grid[0], grid[1], 41)
    plain = _run(ps, tr, pp, None, bin=bin, k_window=k_window)
    dd = _run(ps, tr, pp, ps.Dose(electrons_per_probe=1e3, keep_intensity=True), bin=bin, k_window=k_window)
    assert plain.counts is None and plain.dose is None
    assert dd.intensity.shape == plain.intensity.shape == dd.counts.shape
    err = (np.abs(dd.intensity - plain.intensity) / plain.intensity.max(axis=(-2, -1), keepdims=True)).max()
    print(f"grid {grid} window {k_window} bin {bin}: max diff / pattern max {err:.3e}")
    assert err <= 1e-6
    assert np.array_equal(dd.kxs, plain.kxs) and np.array_equal(dd.kys, plain.kys)


# ------------------------------------------------------------------ 3. reproducibility
def test_counts_depend_on_the_seed_and_not_on_the_probe_batch(ps, base):
    tr, pp, dd = base
    again = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED))
    assert again.intensity is None                                      # keep_intensity=False: counts only
    assert np.array_equal(again.counts, dd.counts)
    assert np.array_equal(again.pacbed(), dd.counts.astype(np.float64).mean(axis=0))
    whole = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED), probe_batch=5)
    assert np.array_equal(whole.counts, dd.counts)
    other = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED + 1))
    lit = dd.counts > 0
    assert (other.counts != dd.counts)[lit].mean() > 0.5


def test_detectors_ride_along_noise_free(ps, base):
    tr, pp, dd = base
    dets = [ps.Detector("bf", outer=MRAD), ps.Detector("adf", inner=40.0, outer=150.0)]
    with_dose = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED), detectors=dets)
    calc = ps.MultisliceCalculator(progress=False, detectors=dets, probe_batch=2, frame_batch=2)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    assert np.array_equal(with_dose.stem.signals, calc.run_detectors().signals)
    assert np.array_equal(with_dose.counts, dd.counts)


# ------------------------------------------------------------------ 4. physics
def test_total_counts_follow_the_dose(ps, base):
    """the counts of a probe add up to a Poisson variate of mean N_e * sum(intensity) / I_incident <= N_e: within 5 sqrt(N_e)"""
    tr, pp, dd = base
    want = N_E * dd.intensity.sum(axis=(-2, -1)) / dd.incident
    got = dd.counts.astype(np.float64).sum(axis=(-2, -1))
    print("electrons counted per probe", got, "expected", np.round(want, 1))
    assert np.all(want > 0.9 * N_E) and np.all(want < N_E * (1 + 1e-5))
    assert np.all(np.abs(got - want) <= 5.0 * math.sqrt(N_E))


def test_low_dose_counts_are_zero_or_one(ps, base):
    tr, pp, dd = base
    n_e = 0.9e-3 * dd.incident / dd.intensity.max()
    low = _run(ps, tr, pp, ps.Dose(electrons_per_probe=n_e, seed=3, keep_intensity=True))
    assert _expected(low).max() < 1e-3
    assert set(np.unique(low.counts).tolist()) <= {0, 1}


def test_vacuum_counts_stay_inside_the_aperture(ps):
    """no atom in any slice (the two atoms of the cell stand above the stack, where the slice rule drops them): the exit pattern
    is the aperture disc, and so is every count"""
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(32, 5)
    pos = np.tile(np.array([[1.0, 1.0, box[2, 2] + 5.0], [2.0, 2.0, box[2, 2] + 6.0]]), (T, 1, 1))
    tr = ps.Trajectory(atom_types=np.array([5, 7]), positions=pos, velocities=np.zeros_like(pos), box_matrix=box, timestep=0.005)
    pp = [(0.4, 1.1), (1.6, 2.0), (2.9, 0.3)]
    dd = _run(ps, tr, pp, ps.Dose(electrons_per_probe=1e4, seed=8, keep_intensity=True))
    kx, ky = np.fft.fftshift(np.fft.fftfreq(32, dd.pixel[0])), np.fft.fftshift(np.fft.fftfreq(32, dd.pixel[1]))
    disc = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2) < MRAD * 1e-3 / wavelength(EV)
    assert dd.incident == disc.sum()
    assert np.abs(dd.intensity[:, disc] - 1.0).max() < 1e-4
    assert not dd.counts[:, ~disc].any()
    assert np.all(dd.counts[:, disc] > 0)                              # lam = 1e4 / (pixels of the disc), some hundreds each
    got = dd.counts.astype(np.float64).sum(axis=(-2, -1))
    assert np.all(np.abs(got - 1e4) <= 5.0 * math.sqrt(1e4))


# ------------------------------------------------------------------ 5. the library's errors
def test_library_errors_leave_the_handle_usable(ps):
    import ctypes as C
    import torch
    from pyslice_amd import _native
    eng = _native.Engine(6, 8, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    lib, h, ptr = eng._lib, eng._h, _native._ptr
    try:
        d = torch.ones((2, 3, 50), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        p = d.data_ptr()
        out = np.zeros(2 * 48, dtype=np.uint32)
        assert lib.msl_dose_counts(h, 2, 1.0, 1, 0, ptr(out), None) == _native.MSL_ERR_STATE          # before a reset
        assert lib.msl_dose_add(h, p, 2, 3, 48, 50, 0, 3, 6, 8, 1, 1) == _native.MSL_ERR_STATE
        assert lib.msl_dose_reset(h, 2, 0, 8) == _native.MSL_ERR_INVALID
        assert lib.msl_dose_reset(h, 2, 6, 8) == _native.MSL_OK
        assert lib.msl_dose_add(h, p, 2, 3, 48, 50, 0, 3, 6, 8, 1, 1) == _native.MSL_OK
        assert lib.msl_dose_counts(h, 3, 1.0, 1, 0, ptr(out), None) == _native.MSL_ERR_INVALID        # B beyond the reset
        assert b"reset" in lib.msl_last_error(h)
        assert lib.msl_dose_counts(h, 2, -1.0, 1, 0, ptr(out), None) == _native.MSL_ERR_INVALID       # a negative scale
        assert lib.msl_dose_counts(h, 2, float("nan"), 1, 0, ptr(out), None) == _native.MSL_ERR_INVALID
        assert lib.msl_dose_counts(h, 2, float("inf"), 1, 0, ptr(out), None) == _native.MSL_ERR_INVALID
        assert lib.msl_dose_counts(h, 2, 1.0, 1, 2 ** 32 - 1, ptr(out), None) == _native.MSL_ERR_INVALID      # probe word overflows
        assert lib.msl_dose_counts(h, 2, 1.0, 1, 0, None, None) == _native.MSL_ERR_INVALID
        for bx, by in ((4, 1), (1, 3), (0, 1)):                          # a bin that does not divide the window
            assert lib.msl_dose_add(h, p, 2, 3, 48, 50, 0, 3, 6, 8, bx, by) == _native.MSL_ERR_INVALID
        assert lib.msl_dose_add(h, p, 2, 3, 48, 50, 0, 3, 6, 8, 2, 2) == _native.MSL_ERR_INVALID      # not the reset's 6 x 8 pixels
        assert lib.msl_dose_add(h, p, 3, 3, 48, 50, 0, 3, 6, 8, 1, 1) == _native.MSL_ERR_INVALID      # more probes than the reset
        assert lib.msl_dose_add(h, p, 2, 3, 48, 50, 2, 2, 6, 8, 1, 1) == _native.MSL_ERR_INVALID      # frame range leaves [0, T)
        assert out.sum() == 0                                            # no refused call wrote anything
        # every refusal left the accumulator as the one successful add made it: 3 frames of |1|^2
        acc = np.zeros((2, 6, 8))
        assert lib.msl_dose_counts(h, 2, 2.0, 1, 0, ptr(out), ptr(acc)) == _native.MSL_OK
        assert np.array_equal(acc, np.full((2, 6, 8), 3.0))
        assert np.array_equal(out.reshape(2, 6, 8), ps.poisson_counts(acc * 2.0, 1, np.arange(2)))
        # an expected count that is not finite is found by the kernel: the flag word comes back with the counts
        bad = torch.ones((2, 3, 50), dtype=torch.complex64, device="cuda")
        bad[1, 2, 17] = float("nan")
        torch.cuda.synchronize()
        eng.dose_reset(2, (6, 8))
        eng.dose_add(0, 3, src=(bad.data_ptr(), 2, 3, 6, 8, 50))
        assert lib.msl_dose_counts(h, 2, 1.0, 1, 0, ptr(out), None) == _native.MSL_ERR_INVALID
        assert b"not finite" in lib.msl_last_error(h)
        with pytest.raises(ValueError):
            eng.dose_counts(1.0, 1)
        assert lib.msl_dose_counts(h, 1, 1.0, 1, 0, ptr(out), None) == _native.MSL_OK                 # probe 0 alone is fine
        eng.dose_reset(2, (3, 2))
        eng.dose_add(0, 3, bin=(2, 4), src=(p, 2, 3, 6, 8, 50))
        counts, acc = eng.dose_counts(1.0, 4, keep_intensity=True)
        assert np.array_equal(acc, np.full((2, 3, 2), 24.0)) and np.array_equal(counts, ps.poisson_counts(acc, 4, np.arange(2)))
    finally:
        eng.close()
