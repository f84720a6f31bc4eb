"""Thickness series on the MI355X: spectra of intermediate layers (MultisliceCalculator(layers=...), msl_set_layers).

Layer k = the wave after the transmission of slice k, i.e. the exit wave of the stack cut after slice k:
oracle.diffraction(oracle.propagate(probes, V[:, :, :k+1], xs, ys, zs[:k+1], eV)).  Same contract as the exit wave
(tests/test_gpu_parity.py): rel-L2 <= 1e-4 and the reference's residual <= 1e-6; TACAW rel-L2 <= 2e-4."""
import os

import numpy as np
import pytest

from conftest import ref_residual, rel_l2

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4
RESID_TOL = 1e-6
TACAW_TOL = 2e-4
EV, MRAD = 100e3, 30.0


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import multislice_oracle
    return multislice_oracle


def _workers(orc):
    return min(16, orc.usable_cores())


def oracle_layers(orc, tr, pp, layers, frames=None):
    """(P, T, nx, ny, L) complex128: diffraction of the stack cut after each slice index of `layers`"""
    xs, ys, zs, *_ = orc.grid_from_box(tr.box_matrix)
    pr = orc.batched_probes(orc.probe_array(xs, ys, MRAD, EV), xs, ys, pp)
    frames = list(range(tr.positions.shape[0])) if frames is None else list(frames)
    w = _workers(orc)
    out = np.zeros((len(pp), len(frames), len(xs), len(ys), len(layers)), dtype=np.complex128)
    for ti, t in enumerate(frames):
        V = orc.potential(xs, ys, zs, tr.positions[t], tr.atom_types)
        for li, k in enumerate(layers):
            ex = orc.propagate(pr, V[:, :, :k + 1], xs, ys, zs[:k + 1], EV, workers=w)
            out[:, ti, :, :, li] = orc.diffraction(ex, workers=w)
    return out


def _probes(tr, P, seed):
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    return [tuple(v) for v in np.random.default_rng(seed).random((P, 2)) * [lx, ly]]


# ------------------------------------------------------------------ every slice-loop family and work-buffer layout
@pytest.mark.parametrize("nx,ny,nz,P,layers", [
    (256, 256, 7, 2, [0, 2, 3, 5]),          # scheme A, R = 16, interleaved order; 5 = nz - 2 writes natural order
    (1024, 256, 6, 2, [0, 1, 2, 4]),         # scheme A, R = 32 / 16
    (256, 1024, 5, 1, [0, 1, 3]),
    (512, 512, 5, 2, [0, 1, 2, 3]),          # rowT2 (scheme B, interleaved)
    (600, 500, 4, 2, [0, 1, 2]),             # rowTM
    (1000, 256, 4, 1, [0, 1, 2]),            # rowTM2
    (2048, 2048, 6, 2, [0, 1, 2, 4]),        # 2048-point wave per line, paired-lines layout
    (501, 491, 4, 2, [0, 1, 2]),             # convolution kernels, natural order
])
def test_layers_match_the_truncated_stack_on_every_loop(ps, orc, nx, ny, nz, P, layers):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.04, seed=nx + 7 * ny)
    pp = _probes(tr, P, nx + ny)
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64", layers=layers)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    assert (calc.nx, calc.ny, calc.nz) == (nx, ny, nz)
    wf = calc.run()
    got = npy(wf.wavefunction_data)
    want_layers = list(layers) + [nz - 1]
    assert got.shape == (P, 1, nx, ny, len(want_layers))
    assert list(wf.layer) == want_layers
    want = oracle_layers(orc, tr, pp, want_layers)
    for li, k in enumerate(want_layers):
        assert rel_l2(got[..., li], want[..., li]) < WAVE_TOL, (k, rel_l2(got[..., li], want[..., li]))
        assert ref_residual(got[..., li], want[..., li]) < RESID_TOL, k


def _engine_case(ps, orc, nx, ny, nz, P, fft_path, layers, seed=5):
    """Engine on an uploaded oracle potential: layered result (L, P, nx, ny) and the oracle's"""
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import loadKirkland, slice_edges
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.05, seed=seed)
    xs, ys, zs, *_ = orc.grid_from_box(tr.box_matrix)
    pp = _probes(tr, P, seed)
    V = orc.potential(xs, ys, zs, tr.positions[0], tr.atom_types)
    eng = _native.Engine(nx, ny, nz, xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(EV), interaction_sigma(EV),
                         n_probes=P, n_frames=1, fft_path=fft_path)
    eng.set_kirkland(loadKirkland())
    eng.set_slices(*slice_edges(np.asarray(zs, dtype=np.float64)))
    eng.set_probes(MRAD, np.asarray(pp, dtype=np.float64))
    eng.upload_potential(np.ascontiguousarray(np.moveaxis(V, 2, 0)).astype(np.float32))
    eng.set_layers(layers)
    eng.propagate_frame(0)
    eng.synchronize()
    return eng, tr, pp, oracle_layers(orc, tr, pp, list(layers) + [nz - 1])


@pytest.mark.parametrize("nx,ny,nz,fft_path", [(96, 80, 5, 1), (256, 128, 5, 1), (256, 128, 6, 0)])
def test_layers_on_the_two_pass_loop_and_the_abi(ps, orc, nx, ny, nz, fft_path):
    """fft_path = 1: the two-pass loop (row launch, then column launch per slice); the tap takes the row launch's
    P_y fft_y psi_k.  Also the ABI of the layered result: buffer size, dense download, complex128 download."""
    from pyslice_amd import _native
    P, layers = 2, [0, 1, 3]
    eng, tr, pp, want = _engine_case(ps, orc, nx, ny, nz, P, fft_path, layers)
    L = len(layers) + 1
    assert eng.n_layers == L
    pitch = eng.result_pitch(_native.BUF_LAYERS)
    assert pitch == eng.result_pitch(_native.BUF_WAVEFUNCTION) and pitch >= nx * ny
    assert eng.buffer_bytes(_native.BUF_LAYERS) == L * P * 1 * pitch * 8
    assert eng.buffer_bytes(_native.BUF_WAVEFUNCTION) == P * 1 * pitch * 8
    dense = eng.layers_c64()                                     # (L, P, T, nx, ny)
    assert dense.shape == (L, P, 1, nx, ny)
    got = np.moveaxis(dense, 0, -1)                              # (P, T, nx, ny, L)
    for li in range(L):
        assert rel_l2(got[..., li], want[..., li]) < WAVE_TOL, li
        assert ref_residual(got[..., li], want[..., li]) < RESID_TOL, li
    c128 = eng.layers_c128(1)
    assert c128.dtype == np.complex128 and c128.shape == (P, 1, nx, ny, L)
    np.testing.assert_array_equal(c128, got.astype(np.complex128))
    # the exit block is the wavefunction buffer every single-layer entry point reads
    np.testing.assert_array_equal(eng.wavefunction(), dense[-1])
    # back to a single layer: the result buffer shrinks to one block
    eng.set_layers([])
    assert eng.n_layers == 1 and eng.buffer_bytes(_native.BUF_LAYERS) == P * pitch * 8
    eng.close()


def test_set_layers_rejects_bad_indices_and_open_streams(ps):
    from pyslice_amd import _native
    eng = _native.Engine(64, 64, 6, 0.1, 0.1, 0.5, 0.037, 0.0008, n_probes=1, n_frames=4)
    for bad in ([2, 1], [1, 1], [-1], [5], [0, 6]):
        with pytest.raises(ValueError, match="msl_set_layers"):
            eng.set_layers(bad)
    assert eng.n_layers == 1
    eng.set_layers([0, 4])
    assert eng.buffer_bytes(_native.BUF_LAYERS) == 3 * eng.buffer_bytes(_native.BUF_WAVEFUNCTION)
    eng.tacaw_stream_begin(4)
    with pytest.raises(RuntimeError, match="stream"):
        eng.set_layers([1])
    eng.close()
    helper = _native.Engine(64, 64, 6, 0.1, 0.1, 0.5, 0.037, 0.0008, n_probes=1, n_frames=0)
    with pytest.raises(RuntimeError, match="n_frames"):
        helper.set_layers([1])
    helper.close()


def test_layers_too_large_for_the_device_fail_in_setup(ps):
    """L x P x T x pitch x 8 B beyond the free device memory: MemoryError naming the layers, before any allocation"""
    import torch
    from pyslice_amd.synthetic import synthetic_trajectory
    free_b = torch.cuda.mem_get_info(0)[0]
    nz, T = 40, 64
    per_layer = 16 * T * 1024 * 1024 * 8
    L = int(free_b // per_layer) + 2
    if L > nz:
        pytest.skip(f"{free_b / 1e9:.0f} GB free: would need more than {nz} layers")
    tr = synthetic_trajectory(1024, nz, T, density=0.001, seed=2)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [(lx * (i + 0.5) / 16, ly / 2) for i in range(16)]
    calc = ps.MultisliceCalculator(progress=False, layers=list(range(L - 1)))
    with pytest.raises(MemoryError, match="layers"):
        calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    assert calc._engine is None


# ------------------------------------------------------------------ calculator: frame batching, windows, output modes
@pytest.fixture(scope="module")
def series(ps, orc):
    """5 frames x 2 probes on 256 x 192 x 6 slices; layers [3, 1, 1, 0] -> [0, 1, 3, 5]"""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(256, 6, 5, ny=192, density=0.05, seed=31)
    pp = _probes(tr, 2, 8)
    layers = [0, 1, 3, 5]
    return tr, pp, layers, oracle_layers(orc, tr, pp, layers)


def _run(ps, tr, pp, **kw):
    calc = ps.MultisliceCalculator(progress=False, **kw)
    calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    return calc, calc.run()


@pytest.mark.parametrize("fb", [2, 1])
def test_calculator_layers_frame_batching_and_output_modes(ps, series, fb):
    tr, pp, layers, want = series
    calc, wf = _run(ps, tr, pp, frame_batch=fb, layers=[3, 1, 1, 0])
    assert calc._engine.frame_batch == fb
    got = npy(wf.wavefunction_data)
    assert got.dtype == np.complex128 and got.shape == (2, 5, 256, 192, 4)
    assert isinstance(wf.layer, np.ndarray) and wf.layer.dtype.kind == "i" and list(wf.layer) == layers
    for li in range(4):
        assert rel_l2(got[..., li], want[..., li]) < WAVE_TOL, li
        assert ref_residual(got[..., li], want[..., li]) < RESID_TOL, li
    # the exit layer is bit-identical to the same run without layers
    _, plain = _run(ps, tr, pp, frame_batch=fb)
    np.testing.assert_array_equal(got[..., -1], npy(plain.wavefunction_data)[..., 0])
    # complex64 host and the zero-copy device view hold the same values
    _, wf64 = _run(ps, tr, pp, frame_batch=fb, layers=[3, 1, 1, 0], dtype="complex64")
    g64 = npy(wf64.wavefunction_data)
    assert g64.dtype == np.complex64 and g64.shape == got.shape
    np.testing.assert_array_equal(g64.astype(np.complex128), got)
    cd, wfd = _run(ps, tr, pp, frame_batch=fb, layers=[3, 1, 1, 0], output="device")
    dev = wfd.wavefunction_data
    assert dev.is_cuda and tuple(dev.shape) == got.shape
    assert dev.data_ptr() == cd._engine.device_ptr(ps._native.BUF_LAYERS)           # a view of the library buffer, not a copy
    np.testing.assert_array_equal(npy(dev), g64)


@pytest.mark.parametrize("window,kbin", [((64, 48), None), ((64, 48), (2, 3)), ((128, 96), (4, 4))])
def test_calculator_layers_with_k_window_and_k_bin(ps, series, window, kbin):
    tr, pp, layers, want = series
    _, wf = _run(ps, tr, pp, frame_batch=2, layers=layers[:-1], k_window=window, k_bin=kbin, dtype="complex64")
    got = npy(wf.wavefunction_data)
    wx, wy = window
    x0, y0 = 256 // 2 - wx // 2, 192 // 2 - wy // 2
    ref = want[:, :, x0:x0 + wx, y0:y0 + wy, :]
    if kbin is not None:
        bx, by = kbin
        P, T = ref.shape[:2]
        ref = ref.reshape(P, T, wx // bx, bx, wy // by, by, 4).sum(axis=(3, 5))
    assert got.shape == ref.shape
    for li in range(4):
        assert rel_l2(got[..., li], ref[..., li]) < WAVE_TOL, li


def test_tacaw_and_haadf_on_a_layered_result(ps, orc, series):
    tr, pp, layers, want = series
    _, wf = _run(ps, tr, pp, frame_batch=2, layers=layers[:-1])
    time = wf.time
    for li in range(len(layers)):
        tac = ps.TACAWData(wf, layer_index=li)
        assert tac._intensity_src[1] is None                   # the engine's own buffer: no host round trip
        f, inten = orc.tacaw(want, time, layer_index=li)
        ti = npy(tac.intensity)
        assert rel_l2(ti, inten) < TACAW_TOL, li
        if li == 1:                                            # reductions after an intermediate layer's transform
            assert rel_l2(tac.spectrum(), orc.tacaw_spectrum(inten)) < TACAW_TOL
            assert rel_l2(tac.spectrum(probe_index=1), orc.tacaw_spectrum(inten, probe_index=1)) < TACAW_TOL
            assert rel_l2(tac.diffraction(), orc.tacaw_diffraction(inten)) < TACAW_TOL
            assert rel_l2(tac.diffraction(probe_index=0), orc.tacaw_diffraction(inten, probe_index=0)) < TACAW_TOL
    # the default layer is the exit wave
    tac = ps.TACAWData(wf)
    _, inten = orc.tacaw(want, time)
    assert rel_l2(npy(tac.intensity), inten) < TACAW_TOL
    np.testing.assert_array_equal(npy(tac.intensity), npy(ps.TACAWData(wf, layer_index=len(layers) - 1).intensity))
    # HAADF reads the exit layer: the same image as an unlayered run
    _, wfl = _run(ps, tr, pp, frame_batch=2, layers=layers[:-1])
    _, plain = _run(ps, tr, pp, frame_batch=2)
    np.testing.assert_array_equal(ps.HAADFData(wfl).calculateADF(30.0), ps.HAADFData(plain).calculateADF(30.0))
