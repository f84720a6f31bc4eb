"""Detector response on the MI355X: the device's frames (csrc/camera.h behind msl_camera_frames / msl_dose_frames) against the
definition (pyslice_amd/camera.py) -- bit for bit without readout noise, within the licence of test_gpu_dose.py with it --, the
calculator option, reproducibility over seeds and probe batches, and the library's error codes.

The kernel's tile is 16 (ix) x 64 (iy) outputs per workgroup, staged with a halo of the radius class (0, 1, 2, 4, 8).  The shapes
of test_camera_host.GPU_SHAPES: (3, 45, 63, 2) partial tiles and an asymmetric PSF; (2, 5, 7, 8) a PSF wider than the pattern;
(1, 1, 1, 0); (2, 32, 32, 1); (2, 37, 150, 3) both extents above the tile plus halo (24, 72) and a multiple of neither, 3 x 3 tiles
per pattern, radius 3 in the class of radius 4.
Calculator runs: 48 x 40 and 32 x 32 pixels of 0.1 A, 5 slices, 3 frames at a frame batch of 2, 5 probes, as test_gpu_dose.py."""
import numpy as np
import pytest

from test_camera_host import GPU_NOISE, GPU_PROBE0, GPU_SEED, GPU_SHAPES, camera_case, near_ties

pytestmark = pytest.mark.gpu

EV, MRAD, T = 100e3, 30.0, 3
N_E, SEED = 2.0e4, 5


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


@pytest.fixture(scope="module")
def eng(ps):
    from pyslice_amd import _native
    e = _native.Engine(6, 8, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    yield e
    e.close()


def _cell(ps, nx, ny, seed, P=5):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, 5, T, ny=ny, density=0.1, seed=seed)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(seed + 1).random((P, 2)) * [lx, ly]]
    return tr, pp


def _run(ps, tr, pp, dose, camera=None, bin=(1, 1), probe_batch=2, frame_batch=2, k_window=None):
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=bin, dose=dose, camera=camera), probe_batch=probe_batch,
                                   frame_batch=frame_batch, k_window=k_window)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    assert calc.probe_batch == min(probe_batch, len(pp)) and calc._engine.frame_batch == frame_batch
    return calc.run_diffraction()


def _camera(ps, **kw):
    return ps.Camera(ps.gaussian_psf(0.8), gain=2.5, offset=20, **kw)


# ------------------------------------------------------------------ 1. noise-free, bit for bit
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_noise_free_frames_are_the_definition_bit_for_bit(ps, eng, shape):
    counts, cam = camera_case(shape)
    eng.set_camera(cam)
    got = eng.camera_frames(counts, seed=GPU_SEED, probe0=0)
    want = ps.camera_frames(counts, cam, GPU_SEED, np.arange(shape[0]))
    assert got.dtype == np.uint16 and got.shape == counts.shape
    differ = int((got != want).sum())
    print(f"shape {shape}: {differ} of {want.size} pixels differ; frames in [{want.min()}, {want.max()}]")
    assert differ == 0
    if want.size > 100:
        assert want.max() == 65535 and want.min() < 300 and len(np.unique(want)) > 50       # the case clips and resolves
    assert np.array_equal(eng.camera_frames(counts, seed=1, probe0=99), got)                # nothing is drawn without noise


# ------------------------------------------------------------------ 2. with noise
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_noisy_frames_differ_only_at_near_ties(ps, eng, shape):
    """licensed: a last-place difference of log, sqrt or cos that flips a rounding -- every differing pixel differs by exactly 1,
    is a near-tie (e within 1e-9 max(1, |e|) of a half-integer), and there are at most max(1, 1e-4 n) of them"""
    from pyslice_amd.camera import camera_signal
    counts, cam = camera_case(shape, readout_noise=GPU_NOISE)
    probes = GPU_PROBE0 + np.arange(shape[0])
    eng.set_camera(cam)
    got = eng.camera_frames(counts, seed=GPU_SEED, probe0=GPU_PROBE0)
    want = ps.camera_frames(counts, cam, GPU_SEED, probes)
    quiet = ps.camera_frames(counts, camera_case(shape)[1], GPU_SEED, probes)
    bad = got != want
    differ = int(bad.sum())
    print(f"shape {shape}: {differ} of {want.size} pixels differ")
    assert (want != quiet).mean() > 0.5 or want.size < 10          # the noise is there
    assert np.all(np.abs(got.astype(np.int64) - want.astype(np.int64))[bad] == 1)
    assert np.all(near_ties(camera_signal(counts, cam, GPU_SEED, probes))[bad])
    assert differ <= max(1, int(1e-4 * want.size))
    if want.size > 100:
        assert (eng.camera_frames(counts, seed=GPU_SEED, probe0=GPU_PROBE0 + 1) != got).mean() > 0.5
        assert (eng.camera_frames(counts, seed=GPU_SEED + 1, probe0=GPU_PROBE0) != got).mean() > 0.5


# ------------------------------------------------------------------ 3. + 7. through the calculator
@pytest.fixture(scope="module")
def cells(ps):
    return {}


def _through(ps, cells, grid, k_window, bin):
    """the run with Camera(keep_counts=True), the same run without a camera, and the frames of other probe batches"""
    key = (grid, k_window, bin)
    if key not in cells:
        tr, pp = _cell(ps, grid[0], grid[1], 31)
        dose = ps.Dose(electrons_per_probe=N_E, seed=SEED)
        kept = _run(ps, tr, pp, dose, _camera(ps, keep_counts=True), bin=bin, k_window=k_window)
        plain = _run(ps, tr, pp, dose, None, bin=bin, k_window=k_window)
        cells[key] = (tr, pp, kept, plain)
    return cells[key]


@pytest.mark.parametrize("grid,k_window,bin", [((48, 40), None, (1, 1)), ((32, 32), (15, 15), (1, 1)), ((48, 40), None, (2, 2))])
def test_calculator_frames_are_the_definition_of_its_counts(ps, cells, grid, k_window, bin):
    """the second case stores an odd row length (the 8-byte load path of the pattern pass), the third bins 2 x 2"""
    tr, pp, kept, plain = _through(ps, cells, grid, k_window, bin)
    mx, my = ((grid if k_window is None else k_window)[0] // bin[0], (grid if k_window is None else k_window)[1] // bin[1])
    assert kept.frames.shape == (5, mx, my) and kept.frames.dtype == np.uint16 and kept.counts.dtype == np.uint32
    assert kept.intensity is None and kept.camera.keep_counts and plain.frames is None and plain.camera is None
    assert np.array_equal(kept.counts, plain.counts)
    assert kept.counts.max() > 50
    assert np.array_equal(kept.frames, ps.camera_frames(kept.counts, kept.camera, SEED, np.arange(5)))
    three = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED), _camera(ps), bin=bin, k_window=k_window, probe_batch=3)
    assert np.array_equal(three.frames, kept.frames)
    assert three.counts is None and three.intensity is None and three.frames.dtype == np.uint16
    assert np.array_equal(three.pacbed(), ((kept.frames.astype(np.float64) - 20.0) / 2.5).mean(axis=0))


def test_keep_intensity_rides_along(ps, cells):
    tr, pp, kept, plain = _through(ps, cells, (48, 40), None, (1, 1))
    both = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED, keep_intensity=True), _camera(ps))
    ref = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED, keep_intensity=True))
    assert both.counts is None and np.array_equal(both.frames, kept.frames) and np.array_equal(both.intensity, ref.intensity)


# ------------------------------------------------------------------ 4. readout noise in a run
def test_noisy_run_depends_on_the_seed_and_not_on_the_probe_batch(ps, cells):
    tr, pp, kept, plain = _through(ps, cells, (48, 40), None, (1, 1))
    cam = _camera(ps, readout_noise=3.0)
    two = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED), cam, probe_batch=2)
    five = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED), cam, probe_batch=5)
    assert np.array_equal(two.frames, five.frames)
    assert (two.frames != kept.frames).mean() > 0.5
    other = _run(ps, tr, pp, ps.Dose(electrons_per_probe=N_E, seed=SEED + 1), cam, probe_batch=5)
    assert (other.frames != two.frames).mean() > 0.5
    want = ps.camera_frames(kept.counts, cam, SEED, np.arange(5))
    differ = int((want != two.frames).sum())
    print(f"{differ} of {want.size} pixels differ from the definition")
    assert differ <= max(1, int(1e-4 * want.size))


# ------------------------------------------------------------------ 5. the identity camera
def test_identity_camera_through_dose_frames(ps, eng):
    import torch
    B, wx, wy = 3, 6, 8
    rng = np.random.default_rng(12)
    W = (rng.standard_normal((B, 2, wx * wy)) + 1j * rng.standard_normal((B, 2, wx * wy))).astype(np.complex64)
    W *= np.repeat(10.0 ** np.linspace(-1.0, 2.5, wx), wy).astype(np.float32)[None, None, :]       # the last rows count above 65535
    d = torch.from_numpy(W).cuda()
    torch.cuda.synchronize()
    eng.dose_reset(B, (wx, wy))
    eng.dose_add(0, 2, src=(d.data_ptr(), B, 2, wx, wy))
    counts, acc = eng.dose_counts(3.0, 9, probe0=4, B=B, keep_intensity=True)
    assert counts.max() > 65535 and counts.min() < 10
    eng.set_camera(ps.Camera())
    frames, cnt, sums = eng.dose_frames(3.0, 9, probe0=4, B=B, keep_counts=True, keep_intensity=True)
    assert np.array_equal(cnt, counts) and np.array_equal(sums, acc)
    assert np.array_equal(frames, np.minimum(counts, 65535).astype(np.uint16))
    only, none_c, none_i = eng.dose_frames(3.0, 9, probe0=4, B=B)
    assert none_c is None and none_i is None and np.array_equal(only, frames)
    assert np.array_equal(eng.dose_counts(3.0, 9, probe0=4, B=B)[0], counts)                       # msl_dose_counts as it was


# ------------------------------------------------------------------ 6. the library's errors
def test_library_errors_leave_the_handle_usable(ps):
    import torch
    from pyslice_amd import _native
    eng = _native.Engine(6, 8, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    lib, h, ptr = eng._lib, eng._h, _native._ptr
    INVALID, STATE, OK = _native.MSL_ERR_INVALID, _native.MSL_ERR_STATE, _native.MSL_OK
    try:
        counts = np.arange(2 * 48, dtype=np.uint32).reshape(2, 6, 8)
        frames = np.zeros((2, 6, 8), dtype=np.uint16)
        cnt_out = np.zeros((2, 6, 8), dtype=np.uint32)
        assert lib.msl_camera_frames(h, ptr(counts), 2, 6, 8, 1, 0, ptr(frames)) == STATE             # no camera yet
        assert b"camera" in lib.msl_last_error(h)
        assert lib.msl_dose_frames(h, 2, 1.0, 1, 0, ptr(frames), None, None) == STATE                 # neither camera nor reset
        psf = np.full((3, 3), 0.1)
        neg, nan, wide = psf.copy(), psf.copy(), np.full((19, 19), 0.001)
        neg[1, 2], nan[0, 0] = -0.1, np.nan
        for args in ((9, ptr(wide), 1.0, 0.0, 0.0, 16), (1, None, 1.0, 0.0, 0.0, 16), (1, ptr(neg), 1.0, 0.0, 0.0, 16),
                     (1, ptr(nan), 1.0, 0.0, 0.0, 16), (1, ptr(psf), 0.0, 0.0, 0.0, 16), (1, ptr(psf), -1.0, 0.0, 0.0, 16),
                     (1, ptr(psf), float("nan"), 0.0, 0.0, 16), (1, ptr(psf), float("inf"), 0.0, 0.0, 16),
                     (1, ptr(psf), 1.0, -1.0, 0.0, 16), (1, ptr(psf), 1.0, float("inf"), 0.0, 16), (1, ptr(psf), 1.0, 0.0, -1.0, 16),
                     (1, ptr(psf), 1.0, 0.0, float("nan"), 16), (1, ptr(psf), 1.0, 0.0, 0.0, 0), (1, ptr(psf), 1.0, 0.0, 0.0, 17)):
            assert lib.msl_set_camera(h, *args) == INVALID, args
        assert lib.msl_camera_frames(h, ptr(counts), 2, 6, 8, 1, 0, ptr(frames)) == STATE             # a refused camera is no camera
        assert lib.msl_set_camera(h, 1, ptr(psf), 2.0, 3.0, 0.0, 12) == OK
        assert lib.msl_dose_frames(h, 2, 1.0, 1, 0, ptr(frames), None, None) == STATE                 # a camera, no reset
        assert b"reset" in lib.msl_last_error(h)
        for args in ((None, 2, 6, 8, 1, 0, ptr(frames)), (ptr(counts), 2, 6, 8, 1, 0, None), (ptr(counts), 0, 6, 8, 1, 0, ptr(frames)),
                     (ptr(counts), 2, 0, 8, 1, 0, ptr(frames)), (ptr(counts), 2, 6, -1, 1, 0, ptr(frames)),
                     (ptr(counts), 2, 6, 8, 1, -1, ptr(frames)), (ptr(counts), 2, 6, 8, 1, 2 ** 32 - 1, ptr(frames))):
            assert lib.msl_camera_frames(h, *args) == INVALID, args
        assert lib.msl_set_camera(h, 1, ptr(psf), 2.0, -3.0, 0.0, 12) == INVALID                     # the camera set before is kept
        assert not frames.any()                                                                       # no refused call wrote anything
        cam = ps.Camera(psf, gain=2.0, offset=3.0, bits=12)
        assert lib.msl_camera_frames(h, ptr(counts), 2, 6, 8, 1, 0, ptr(frames)) == OK
        assert np.array_equal(frames, ps.camera_frames(counts, cam, 1, [0, 1]))
        assert lib.msl_camera_frames(h, ptr(counts), 1, 12, 8, 1, 2 ** 32 - 1, ptr(frames)) == OK     # the last probe index, another shape
        assert np.array_equal(frames.reshape(1, 12, 8), ps.camera_frames(counts.reshape(1, 12, 8), cam, 1, [2 ** 32 - 1]))
        # msl_dose_frames: the checks of msl_dose_counts
        d = torch.ones((2, 3, 50), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        eng.dose_reset(2, (6, 8))
        eng.dose_add(0, 3, src=(d.data_ptr(), 2, 3, 6, 8, 50))
        frames[:] = 0
        assert lib.msl_dose_frames(h, 2, 1.0, 1, 0, None, None, None) == INVALID
        assert lib.msl_dose_frames(h, 3, 1.0, 1, 0, ptr(frames), None, None) == INVALID               # B beyond the reset
        assert lib.msl_dose_frames(h, 2, -1.0, 1, 0, ptr(frames), None, None) == INVALID
        assert lib.msl_dose_frames(h, 2, float("nan"), 1, 0, ptr(frames), None, None) == INVALID
        assert lib.msl_dose_frames(h, 2, 1.0, 1, 2 ** 32 - 1, ptr(frames), None, None) == INVALID     # probe word overflows
        assert not frames.any()
        assert lib.msl_dose_frames(h, 2, 2.0, 1, 0, ptr(frames), ptr(cnt_out), None) == OK
        want = ps.poisson_counts(np.full((2, 6, 8), 6.0), 1, np.arange(2))
        assert np.array_equal(cnt_out, want) and np.array_equal(frames, ps.camera_frames(want, cam, 1, [0, 1]))
        assert lib.msl_set_camera(h, -1, None, 1.0, 0.0, 0.0, 16) == OK                               # cleared
        assert lib.msl_dose_frames(h, 2, 2.0, 1, 0, ptr(frames), None, None) == STATE
        assert lib.msl_dose_counts(h, 2, 2.0, 1, 0, ptr(cnt_out), None) == OK and np.array_equal(cnt_out, want)
        assert lib.msl_set_camera(h, 0, None, 1.0, 0.0, 0.0, 16) == OK                                # NULL with radius 0: the weight 1
        assert lib.msl_dose_frames(h, 2, 2.0, 1, 0, ptr(frames), None, None) == OK and np.array_equal(frames, want.astype(np.uint16))
    finally:
        eng.close()
