"""Windowed, segment-averaged (Welch) TACAW spectra on the MI355X: time_welch_kernel<L> (msl_tacaw_welch) against the float64
definition pyslice_amd.welch.welch_intensity on the same complex64 input.

Every caller-held input is a large constant (4096 - 1500i) plus two tones plus noise, so that a kernel that subtracts only the
line's first sample -- what the unwindowed time kernels do -- fails by orders of magnitude under a tapered window.  Bound: the
project's TACAW_TOL = 2e-4 rel-L2 per image; expected is a few 1e-7, since x - x[first] is exact in fp32 and
everything after it works on numbers of the size of the result."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TACAW_TOL = 2e-4
LENGTHS = [16, 18, 20, 21, 24, 25, 27, 28, 30, 32, 35, 36, 40, 42, 45, 48, 49, 50, 54, 56, 60, 63, 64, 70, 72, 75, 80, 81, 84, 90, 96, 98,
           100, 105, 108, 112, 120, 125, 126, 128]
MRAD, EV = 30.0, 100e3


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


@pytest.fixture(scope="module")
def eng(ps):
    from pyslice_amd import _native
    e = _native.Engine(2, 2, 1, 1.0, 1.0, 1.0, 1.0, 0.0, n_probes=1, n_frames=0, device=0)
    yield e
    e.close()


def make_input(batch, T, npix, seed):
    """(batch, T, npix) complex64: 4096 - 1500i, two tones of per-pixel amplitude and phase, noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)[None, :, None]
    a1, a2 = 0.5 + 2.5 * rng.random((2, batch, 1, npix))
    p1, p2 = 2 * np.pi * rng.random((2, batch, 1, npix))
    x = (4096.0 - 1500.0j) + a1 * np.exp(1j * (2 * np.pi * 0.11 * t + p1)) + a2 * np.exp(-1j * (2 * np.pi * 0.27 * t + p2))
    x = x + 0.3 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    return x.astype(np.complex64)


def device_welch(eng, x, L, hop, window):
    """msl_tacaw_welch on caller-held memory -> (batch, L, npix) float32 on the host"""
    import torch
    from pyslice_amd import welch
    batch, T, npix = x.shape
    src = torch.from_numpy(x).cuda()
    dst = torch.full((batch, L, npix), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.tacaw_welch(L, hop, None if window is None else welch.window(window, L), src.data_ptr(), dst.data_ptr(), batch, T, npix)
    return dst.cpu().numpy()


def check(eng, x, L, hop, window, label):
    from pyslice_amd import welch
    got = device_welch(eng, x, L, hop, window)
    want = welch.welch_intensity(x, L, hop, "boxcar" if window is None else window)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    for b in range(x.shape[0]):
        e = rel_l2(got[b], want[b])
        print(f"{label} image {b}: rel-L2 {e:.3e}")
        assert e < TACAW_TOL, (label, b, e)
    assert np.array_equal(got[:, L // 2], np.zeros_like(got[:, L // 2])), label       # row 0 of the unshifted axis: exactly 0
    return got


# ------------------------------------------------------------------ 1. every kernel once
def test_every_segment_length(eng):
    """all 40 instantiations, one process, one function, stopping at the first failure: T = 2 L + 3 (three segments at hop L // 2
    and a tail), Hann, two images of 300 pixels (one full tile of 256 and a ragged one)"""
    for L in LENGTHS:
        check(eng, make_input(2, 2 * L + 3, 300, L), L, L // 2, "hann", f"L={L}")


# ------------------------------------------------------------------ 2. segment geometry
@pytest.mark.parametrize("L", [48, 25, 105])
def test_segment_geometry_and_windows(eng, L):
    rng = np.random.default_rng(L)
    arr = 0.05 + rng.random(L)
    arr[3] = 0.0                                                                      # (zeros are allowed, negatives are not)
    x1 = make_input(2, L, 300, 100 + L)
    check(eng, x1, L, L // 2, "hann", f"L={L} S=1")                                    # one segment: T = L
    check(eng, make_input(2, 3 * L, 300, 200 + L), L, L, "hann", f"L={L} hop=L")       # Bartlett: three abutting segments
    T, hop = (100, 20) if L == 48 else (2 * L + 7, max(1, (2 * L) // 5))
    xt = make_input(2, T, 300, 300 + L)
    from pyslice_amd import welch
    assert (T - L) % hop != 0 and welch.segments(T, L, hop) >= 2                       # a tail that no full segment covers
    for window in ("boxcar", "hann", "hamming", "blackman", arr, None):
        name = window if isinstance(window, str) else ("None" if window is None else "array")
        check(eng, xt, L, hop, window, f"L={L} T={T} hop={hop} {name}")
    check(eng, xt, L, 1, "hann", f"L={L} T={T} hop=1")                                 # the smallest hop


# ------------------------------------------------------------------ 3. the grid-stride loop
def test_more_tiles_than_workgroups(eng):
    """L = 128 runs one workgroup per CU (one wave per SIMD, 512 registers per lane): 258 tiles of 256 pixels are more than the 256
    CUs of the device hold at once, and the last tile has 7 pixels.  Input about 100 MB."""
    import torch
    L, T, hop = 128, 192, 64
    npix = 257 * 256 + 7
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (npix + 255) // 256 > n_cus, "raise npix: the launch must have more tiles than workgroups"
    rng = np.random.default_rng(3)
    t = np.arange(T, dtype=np.float32)[:, None]
    a = (0.5 + 2.5 * rng.random((2, npix))).astype(np.float32)
    p = (2 * np.pi * rng.random((2, npix))).astype(np.float32)
    x = np.empty((1, T, npix), dtype=np.complex64)
    x[0] = (4096.0 - 1500.0j) + a[0] * np.exp(1j * (np.float32(2 * np.pi * 0.11) * t + p[0])) + a[1] * np.exp(-1j * (np.float32(2 * np.pi * 0.27) * t + p[1]))
    x[0] += (0.3 * (rng.standard_normal((T, npix), dtype=np.float32) + 1j * rng.standard_normal((T, npix), dtype=np.float32))).astype(np.complex64)
    check(eng, x, L, hop, "hann", f"L={L} npix={npix}")


# ------------------------------------------------------------------ 4. consistency with the existing transform
@pytest.mark.parametrize("T", [16, 100, 128])
def test_one_boxcar_segment_equals_msl_tacaw(eng, T):
    import torch
    x = make_input(2, T, 300, 400 + T)
    got = device_welch(eng, x, T, T, None)
    src = torch.from_numpy(x).cuda()
    dst = torch.empty((2, T, 300), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.tacaw(src.data_ptr(), dst.data_ptr(), 2, T, 300)
    old = dst.cpu().numpy()
    for b in range(2):
        e = rel_l2(got[b], old[b])
        print(f"T={T} image {b}: welch(L=T, hop=T, boxcar) against msl_tacaw rel-L2 {e:.3e}")
        assert e < TACAW_TOL, (T, b, e)


# ------------------------------------------------------------------ 8. repeatability, refusals
def test_repeated_calls_are_bitwise_equal(eng):
    x = make_input(2, 100, 300, 9)
    a = device_welch(eng, x, 48, 20, "hann")
    other = device_welch(eng, x, 48, 20, "blackman")                                  # (another table in between)
    b = device_welch(eng, x, 48, 20, "hann")
    assert np.array_equal(a, b) and not np.array_equal(a, other)


def test_library_refusals(eng):
    import torch
    src = torch.zeros((1, 64, 32), dtype=torch.complex64, device="cuda")
    dst = torch.zeros((1, 64, 32), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    for L, hop, w, T in ((32, 16, None, 16), (32, 0, None, 64), (32, 33, None, 64), (32, 16, -np.ones(32), 64), (32, 16, np.zeros(32), 64),
                         (32, 16, None, 1)):
        with pytest.raises(ValueError):
            eng.tacaw_welch(L, hop, w, s, d, 1, T, 32)
    for L in (17, 15, 130):
        with pytest.raises(NotImplementedError):
            eng.tacaw_welch(L, L, None, s, d, 1, 512, 32)
    with pytest.raises(RuntimeError):
        eng.tacaw_welch(32, 16)                                                        # no wavefunction buffer on this handle


# ------------------------------------------------------------------ 5. / 6. handle buffers, pitch, the public interface
@pytest.fixture(scope="module")
def run45(ps):
    """a calculator run on an odd grid: 45 x 35 pixels (1575, at a pitch of 1600), T = 32, P = 2, three slices"""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(45, 3, 32, ny=35, density=0.1, amplitude=0.3, seed=45)
    pp = [(1.1, 0.9), (2.6, 2.2)]
    return tr, pp


def _run(ps, tr, pp, **kw):
    calc = ps.MultisliceCalculator(progress=False, **kw)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    return calc, calc.run()


def _check_reductions(tac, want, label):
    """every reduction of a TACAWData against the same reduction of the float64 intensity `want` (P, L, kx, ky)"""
    P, L = want.shape[:2]
    assert len(tac.frequencies) == L and tuple(npy(tac.intensity).shape) == want.shape
    figures = {"intensity": rel_l2(npy(tac.intensity), want),
               "spectrum()": rel_l2(tac.spectrum(), want.sum(axis=(2, 3)).mean(axis=0)),
               "spectrum(1)": rel_l2(tac.spectrum(1), want[1].sum(axis=(1, 2))),
               "diffraction()": rel_l2(tac.diffraction(), want.sum(axis=1).mean(axis=0))}
    f = float(tac.frequencies[L // 2 + 3])
    figures["spectral_diffraction(f, 0)"] = rel_l2(tac.spectral_diffraction(f, 0), want[0, L // 2 + 3])
    kxs, kys = npy(tac.kxs), npy(tac.kys)
    ix, iy = np.array([3, 10, 22, 40, 44]), np.array([1, 8, 17, 30, 34])
    figures["dispersion"] = rel_l2(tac.dispersion(kxs[ix], kys[iy]), want[:, :, ix, iy].mean(axis=0))
    mask = (np.add.outer(np.arange(want.shape[2]), np.arange(want.shape[3])) % 3 == 0)
    figures["masked_spectrum"] = rel_l2(tac.masked_spectrum(mask), (want * mask).sum(axis=(2, 3)).mean(axis=0))
    figures["spectrum_image"] = rel_l2(tac.spectrum_image(f), want[:, L // 2 + 3].sum(axis=(1, 2)))
    for k, e in figures.items():
        print(f"{label} {k}: rel-L2 {e:.3e}")
        assert e < TACAW_TOL, (label, k, e)
    assert np.array_equal(npy(tac.intensity)[:, L // 2], np.zeros((P,) + want.shape[2:]))


@pytest.mark.parametrize("output", ["host", "device"])
def test_tacaw_data_on_the_resident_result(ps, run45, output):
    from pyslice_amd import welch
    tr, pp = run45
    calc, wf = _run(ps, tr, pp, **({"output": "device"} if output == "device" else {}))
    assert calc._engine.result_pitch() == 1600 and calc._engine.wx * calc._engine.wy == 1575
    waves = npy(wf.wavefunction_data)[..., 0].astype(np.complex64)
    assert waves.shape == (2, 32, 45, 35)
    tac = ps.TACAWData(wf, segment=16, overlap=0.5, window="hann")
    assert (tac.segment, tac.hop, tac.n_segments, tac.window) == (16, 8, 3, "hann")
    assert tac._intensity_src[1] is None and calc._engine.intensity_F == 16       # the engine's own buffer, (P, L, pitch)
    assert np.allclose(tac.frequencies, np.fft.fftshift(np.fft.fftfreq(16, tr.timestep)), rtol=1e-12, atol=0)
    if output == "device":
        assert tac.intensity.is_cuda and tac.intensity.data_ptr() == calc._engine.device_ptr(ps._native.BUF_INTENSITY)     # zero-copy
    _check_reductions(tac, welch.welch_intensity(waves, 16, 8, "hann"), f"resident {output}")
    first = npy(tac.intensity).copy()
    # without a segment nothing changes: the attributes are None and the transform is msl_tacaw's
    plain = ps.TACAWData(wf, window="ignored")
    assert plain.segment is None and plain.hop is None and plain.n_segments is None and plain.window is None
    assert tuple(npy(plain.intensity).shape) == (2, 32, 45, 35) and calc._engine.intensity_F == 32
    assert rel_l2(npy(plain.intensity), welch.welch_intensity(waves, 32, 32, "boxcar")) < TACAW_TOL
    # ... and a segmented transform after it shrinks the buffer again
    again = ps.TACAWData(wf, segment=16, overlap=0.5, window="hann")
    assert calc._engine.intensity_F == 16 and np.array_equal(npy(again.intensity), first)


def test_tacaw_data_on_a_layered_result(ps, run45):
    from pyslice_amd import welch
    tr, pp = run45
    calc, wf = _run(ps, tr, pp, layers=[0])
    waves = npy(wf.wavefunction_data)
    assert waves.shape == (2, 32, 45, 35, 2)
    arr = np.hanning(18)[1:-1] + 0.25                                                # an array window
    for li in (0, 1):
        tac = ps.TACAWData(wf, layer_index=li, segment=16, overlap=0.25, window=arr)
        assert (tac.hop, tac.n_segments) == (12, 2) and np.array_equal(tac.window, arr)
        want = welch.welch_intensity(waves[..., li].astype(np.complex64), 16, 12, arr)
        e = rel_l2(npy(tac.intensity), want)
        print(f"layer {li}: rel-L2 {e:.3e}")
        assert e < TACAW_TOL, (li, e)
    last = npy(tac.intensity).copy()
    exit_default = ps.TACAWData(wf, segment=16, overlap=0.25, window=arr)
    assert np.array_equal(npy(exit_default.intensity), last)                          # the default layer is the exit wave


def test_tacaw_data_on_a_staged_wfdata(ps, run45):
    """a WFData assembled by the user goes through the helper engine: the same numbers as the resident path"""
    from pyslice_amd import welch
    tr, pp = run45
    calc, wf = _run(ps, tr, pp)
    waves = npy(wf.wavefunction_data)
    resident = npy(ps.TACAWData(wf, segment=16, overlap=0.5, window="hann").intensity)
    mine = ps.WFData(probe_positions=list(pp), time=npy(wf.time), kxs=npy(wf.kxs), kys=npy(wf.kys), layer=np.array([0]),
                     wavefunction_data=waves.copy(), probe=None)
    tac = ps.TACAWData(mine, segment=16, overlap=0.5, window="hann")
    assert tac._intensity_src[0] is None                                              # staged: a device copy of its own
    _check_reductions(tac, welch.welch_intensity(waves[..., 0].astype(np.complex64), 16, 8, "hann"), "staged")
    assert np.array_equal(npy(tac.intensity), resident)                               # the same kernel on the same values


# ------------------------------------------------------------------ 7. spectrum image
def test_spectrum_image_with_a_segment(ps):
    from pyslice_amd import welch
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 3, 32, density=0.1, amplitude=0.3, seed=77)
    pp = [(1.0, 1.5), (2.5, 4.0), (4.5, 2.0), (5.5, 5.5)]
    dets = [ps.Detector("bf", outer=MRAD), ps.Detector("adf", inner=35.0, outer=55.0)]

    def spectrum_image(**kw):
        calc = ps.MultisliceCalculator(progress=False, spectroscopy=ps.Spectroscopy(dets, **kw), k_window=(32, 32), probe_batch=2)
        calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
        return calc, calc.run_spectrum_image()
    calc, res = spectrum_image(segment=16, overlap=0.5, window="hann", stem=True)
    assert res.spectra.shape == (4, 16, 2) and res.stem.signals.shape == (4, 32, 2)
    assert np.allclose(res.frequencies, np.fft.fftshift(np.fft.fftfreq(16, tr.timestep)), rtol=1e-12, atol=0)
    _, plain = spectrum_image()
    assert plain.spectra.shape == (4, 32, 2)
    # the waves of the same run, resident, and their detector sums in NumPy
    _, wf = _run(ps, tr, pp, k_window=(32, 32))
    waves = npy(wf.wavefunction_data)[..., 0].astype(np.complex64)
    want = welch.welch_intensity(waves, 16, 8, "hann")
    kx, ky = calc._k_axes()
    for d, det in enumerate(dets):
        m = det.member(kx, ky, wavelength(EV))
        w = (want * m[None, None]).sum(axis=(-2, -1))                                # (4, 16)
        for p in range(4):
            assert np.linalg.norm(w[p]) > 0, det.name
            e = rel_l2(res.spectra[p, :, d], w[p])
            print(f"spectrum image probe {p} {det.name}: rel-L2 {e:.3e}")
            assert e < TACAW_TOL, (det.name, p, e)
        assert np.array_equal(res.spectra[:, 8, d], np.zeros(4))                     # the zero-frequency bin
