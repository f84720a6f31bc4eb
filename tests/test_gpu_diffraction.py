"""Diffraction patterns on the MI355X: msl_diffract against numpy and against the detector pass, run_diffraction() against the
oracle and a known answer, its own probe / frame batching, detectors in the same pass, and a scan whose (P, T, K) result could
not exist on the device."""
import math
import time

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def block_sum(I, bx, by):
    """(..., wx, wy) float64 -> (..., wx/bx, wy/by): the sum of every bx x by block"""
    wx, wy = I.shape[-2:]
    return I.reshape(I.shape[:-2] + (wx // bx, bx, wy // by, by)).sum(axis=(-3, -1))


def _engine(wx, wy):
    from pyslice_amd import _native
    return _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)


# ------------------------------------------------------------------ 1. the kernel alone
KERNEL_CASES = [
    # B, T, (wx, wy), ld pad, bins
    (3, 5, (45, 63), 0, [(1, 1), (3, 7), (5, 9), (45, 63)]),          # odd K: 8-byte loads
    (3, 4, (45, 63), 3, [(1, 1), (3, 7), (5, 9), (45, 63)]),          # odd pad
    (2, 4, (32, 32), 0, [(2, 2), (4, 8), (32, 1)]),                   # 16-byte loads
    (2, 3, (32, 32), 6, [(2, 2), (4, 8), (32, 1)]),                   # even pad: still 16-byte loads
    (2, 3, (32, 32), 5, [(2, 2), (4, 8), (32, 1)]),                   # odd pad: 8-byte loads
    (2, 3, (256, 256), 0, [(8, 8), (2, 64)]),
    (2, 3, (256, 256), 32, [(8, 8), (2, 64)]),
    (1, 3, (600, 600), 0, [(25, 5)]),
    (1, 2, (600, 600), 7, [(25, 5)]),
    (70, 1000, (4, 4), 0, [(1, 1), (2, 2), (4, 4), (1, 4)]),          # B * T > 65535 rows
]


@pytest.mark.parametrize("B,T,shape,ld_pad,bins", KERNEL_CASES)
def test_diffract_kernel_matches_numpy(ps, B, T, shape, ld_pad, bins):
    """msl_diffract on caller-held device memory: every bin is a sum of non-negative terms, held to 1e-6 of itself"""
    import torch
    rng = np.random.default_rng(B * 1000 + T + ld_pad)
    wx, wy = shape
    K, ld = wx * wy, wx * wy + ld_pad
    W = (rng.standard_normal((B, T, K)) + 1j * rng.standard_normal((B, T, K))).astype(np.complex64)
    W *= rng.choice([1e-3, 1.0, 30.0], size=(B, T, 1)).astype(np.float32)
    host = np.full((B, T, ld), np.nan + 1j * np.nan, dtype=np.complex64)      # pad pixels must never be read
    host[:, :, :K] = W
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    I = (np.abs(W.astype(np.complex128)) ** 2).reshape(B, T, wx, wy)
    eng = _engine(wx, wy)
    try:
        src = (dW.data_ptr(), B, T, wx, wy, ld)
        ranges = [(0, 1), (0, min(3, T)), (0, T)] + ([(1, 2)] if T > 2 else []) + ([(T - 1, 1)] if T > 1 else [])
        for bx, by in bins:
            for t0, count in ranges:
                got = eng.diffract(t0=t0, count=count, bin=(bx, by), src=src)
                want = block_sum(I[:, t0:t0 + count].sum(axis=1), bx, by)
                assert got.shape == (B, wx // bx, wy // by)
                err = np.abs(got - want) / want
                print(f"shape {shape} ld+{ld_pad} bin {(bx, by)} frames [{t0},{t0 + count}): max rel err {err.max():.3e}")
                assert err.max() <= 1e-6, (bx, by, t0, count, err.max(), np.unravel_index(err.argmax(), err.shape))
                assert np.array_equal(eng.diffract(t0=t0, count=count, bin=(bx, by), src=src), got)   # no atomics: bitwise reproducible
        assert np.array_equal(eng.diffract(bin=bins[0], src=src), eng.diffract(t0=0, count=T, bin=bins[0], src=src))
    finally:
        eng.close()


def test_diffract_refusals(ps):
    import torch
    eng = _engine(6, 8)
    try:
        d = torch.zeros((2, 3, 50), dtype=torch.complex64, device="cuda")
        p = d.data_ptr()
        assert eng.diffract(bin=(3, 4), src=(p, 2, 3, 6, 8, 50)).shape == (2, 2, 2)
        for kw in (dict(bin=(4, 1), src=(p, 2, 3, 6, 8, 50)),              # bx does not divide wx
                   dict(bin=(1, 3), src=(p, 2, 3, 6, 8, 50)),              # by does not divide wy
                   dict(bin=(0, 1), src=(p, 2, 3, 6, 8, 50)),
                   dict(bin=(1, 1), src=(p, 2, 3, 6, 8, 47)),              # ld < K
                   dict(t0=2, count=2, src=(p, 2, 3, 6, 8, 50)),           # frame range leaves [0, T)
                   dict(t0=-1, count=1, src=(p, 2, 3, 6, 8, 50)),
                   dict(t0=0, count=0, src=(p, 2, 3, 6, 8, 50)),
                   dict(src=(p, 0, 3, 6, 8, 50))):
            with pytest.raises(ValueError):
                eng.diffract(**kw)
        out = np.empty(4, dtype=np.float64)
        from pyslice_amd import _native
        rc = eng._lib.msl_diffract(eng._h, p, 2, 3, 47, 50, 0, 1, 6, 8, 3, 4, _native._ptr(out))     # wx * wy != K
        assert rc == _native.MSL_ERR_INVALID
        with pytest.raises(RuntimeError):
            eng.diffract()                                                   # no wavefunction ring: MSL_ERR_STATE
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. consistency with the detector kernel
def test_unbinned_patterns_agree_with_the_detector_pass(ps):
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.stem_data import detector_bitmask
    from pyslice_amd.synthetic import synthetic_trajectory
    D = ps.Detector
    tr = synthetic_trajectory(64, 5, 3, density=0.1, seed=21)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(23).random((6, 2)) * [lx, ly]]
    dets = [D("bf", outer=25.0), D("abf", inner=12.0, outer=25.0), D("adf", inner=40.0, outer=150.0),
            D("seg", outer=25.0, azimuth=(200.0, 40.0)), D("all")]
    calc = ps.MultisliceCalculator(progress=False, detectors=dets, probe_batch=6, frame_batch=3)
    calc.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
    calc.run_detectors()                                                     # leaves 6 probes x 3 frames in the ring
    eng = calc._engine
    bits = detector_bitmask(dets, *calc._k_axes(), wavelength(100e3))
    for t0, count in ((0, 3), (1, 2), (2, 1)):
        pat = eng.diffract(t0, count, bin=(1, 1))
        assert pat.shape == (6, eng.wx, eng.wy)
        sig = eng.detect(t0, count).sum(axis=1)                              # (6, D) over the same frames
        for d, det in enumerate(dets):
            mine = (pat * ((bits >> d) & 1).astype(np.float64)).sum(axis=(-2, -1))
            err = np.abs(mine - sig[:, d]) / sig[:, d]
            print(f"frames [{t0},{t0 + count}) {det.name}: max rel diff {err.max():.3e}")
            assert err.max() <= 1e-6, det.name
    assert np.array_equal(eng.diffract(0, 3, B=4, bin=(2, 2)), eng.diffract(0, 3, bin=(2, 2))[:4])      # a padded batch


# ------------------------------------------------------------------ 3. the oracle
@pytest.fixture(scope="module")
def oracle_case(ps):
    from oracle import multislice_oracle as orc
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, 3, ny=80, density=0.1, seed=11)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    rng = np.random.default_rng(12)
    pp = [tuple(v) for v in rng.random((20, 2)) * [lx, ly]]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp, workers=orc.usable_cores())
    kx, ky = orc.wf_axes(len(xs), len(ys), 0.1, tr.n_frames, tr.timestep)[:2]
    return tr, pp, want["wavefunction_data"][..., 0], (kx, ky)


@pytest.mark.parametrize("k_window,frame_batch,probe_batch,bin", [(None, 1, 8, (1, 1)), (None, 3, 20, (4, 5)),
                                                                  ((48, 40), 2, 7, (6, 8)), ((33, 27), 2, 7, (3, 9))])
def test_patterns_match_oracle(ps, oracle_case, k_window, frame_batch, probe_batch, bin):
    tr, pp, wf, (okx, oky) = oracle_case
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=bin), probe_batch=probe_batch, k_window=k_window,
                                   frame_batch=frame_batch)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert calc._engine.frame_batch == frame_batch and calc.probe_batch == probe_batch
    dd = calc.run_diffraction()
    nx, ny = wf.shape[-2:]
    kx, ky = np.asarray(okx, dtype=np.float32), np.asarray(oky, dtype=np.float32)
    if k_window is not None:
        x0, y0 = nx // 2 - k_window[0] // 2, ny // 2 - k_window[1] // 2
        wf = wf[..., x0:x0 + k_window[0], y0:y0 + k_window[1]]
        kx, ky = kx[x0:x0 + k_window[0]], ky[y0:y0 + k_window[1]]
    want = block_sum((np.abs(wf.astype(np.complex128)) ** 2).mean(axis=1), *bin)
    assert dd.intensity.shape == want.shape and dd.intensity.dtype == np.float64
    assert dd.bin == bin and dd.n_frames == 3 and dd.stem is None
    errs = [rel_l2(dd.intensity[p], want[p]) for p in range(20)]
    print(f"window {k_window} batches ({frame_batch},{probe_batch}) bin {bin}: max rel-L2 per pattern {max(errs):.3e}")
    assert max(errs) <= 2e-4
    assert np.allclose(npy(dd.kxs), kx.reshape(-1, bin[0]).mean(axis=1), rtol=0, atol=1e-5 * np.abs(kx).max())
    assert np.allclose(npy(dd.kys), ky.reshape(-1, bin[1]).mean(axis=1), rtol=0, atol=1e-5 * np.abs(ky).max())
    assert np.array_equal(dd.pacbed(), dd.intensity.mean(axis=0))


# ------------------------------------------------------------------ 4. known answer
@pytest.mark.parametrize("bin", [(1, 1), (4, 5)])
def test_pattern_total_is_the_aperture_pixel_count(ps, oracle_case, bin):
    """|t| = |P| = 1: the total intensity of every exit spectrum is that of the probe, the number of pixels inside the aperture"""
    from oracle import multislice_oracle as orc
    tr, pp, _, _ = oracle_case
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=bin), probe_batch=8, frame_batch=2)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    dd = calc.run_diffraction()
    nx, ny = len(calc.xs), len(calc.ys)
    kx = np.fft.fftfreq(nx, calc.dx)
    ky = np.fft.fftfreq(ny, calc.dy)
    n_mask = float((np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2) < 30e-3 / orc.wavelength(100e3)).sum())      # the probe's strict mask
    assert n_mask > 50
    assert abs(nx * ny * (np.abs(orc.probe_array(calc.xs, calc.ys, 30.0, 100e3)) ** 2).sum() / n_mask - 1.0) < 1e-12
    tot = dd.intensity.sum(axis=(-2, -1))
    print(f"bin {bin}: totals / aperture pixels - 1 in [{(tot / n_mask - 1).min():.3e}, {(tot / n_mask - 1).max():.3e}]")
    assert np.abs(tot / n_mask - 1.0).max() <= 1e-5


# ------------------------------------------------------------------ 5. probe and frame batches do not change the result
def test_batches_give_the_same_patterns(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 5, 3, density=0.1, seed=21)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(22).random((19, 2)) * [lx, ly]]
    out = {}
    for pb in (1, 7, 19):
        for fb in (1, 2):
            calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=(2, 4)), probe_batch=pb, frame_batch=fb)
            calc.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
            out[pb, fb] = calc.run_diffraction().intensity
    ref = out[19, 2]
    scale = ref.max(axis=(-2, -1), keepdims=True)
    for key, o in out.items():
        err = (np.abs(o - ref) / scale).max()
        print(f"probe_batch, frame_batch {key}: max diff / pattern max {err:.3e}")
        assert err <= 1e-6, key


# ------------------------------------------------------------------ 6. detectors in the same pass
def test_detectors_ride_along(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    D = ps.Detector
    tr = synthetic_trajectory(64, 5, 3, density=0.1, seed=21)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(22).random((19, 2)) * [lx, ly]]
    dets = [D("bf", outer=25.0), D("adf", inner=40.0, outer=150.0), D("haadf", inner=40.0, signal="amplitude"), D("comx", signal="com_x")]
    kw = dict(progress=False, detectors=dets, probe_batch=7, frame_batch=2)
    both = ps.MultisliceCalculator(diffraction=ps.Diffraction(bin=(4, 4)), **kw)
    both.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
    dd = both.run_diffraction()
    only = ps.MultisliceCalculator(**kw)
    only.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
    st = only.run_detectors()
    assert dd.stem is not None and dd.stem.signals.shape == (19, 3, 4)
    assert np.array_equal(dd.stem.signals, st.signals)
    assert [d.name for d in dd.stem.detectors] == [d.name for d in dets]
    assert np.array_equal(both.run_detectors().signals, st.signals)
    # the BF disc chosen after the run, from bins of 4 x 4: the bins whose centre lies inside
    v = dd.virtual(D("bf", outer=25.0))
    assert v.shape == (19,) and (v > 0).all()


# ------------------------------------------------------------------ 7. a scan larger than the device
def test_scan_larger_than_device_memory(ps):
    import torch
    from pyslice_amd import _native
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(512, 4, 1, density=0.05, seed=31)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    K = len(xs) * len(ys)
    assert K == 512 * 512
    P = math.ceil(1.05 * torch.cuda.get_device_properties(0).total_memory / (K * 8))
    rng = np.random.default_rng(32)
    pp = rng.random((P, 2)) * [lx, ly]
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=(16, 16)))
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=[tuple(v) for v in pp])
    eng = calc._engine
    Pc, B = eng.n_probes, eng.frame_batch
    assert P > Pc
    assert eng.buffer_bytes(_native.BUF_WAVEFUNCTION) <= Pc * B * eng.result_pitch() * 8
    t0 = time.time()
    dd = calc.run_diffraction()
    assert time.time() - t0 < 120.0
    assert dd.intensity.shape == (P, 32, 32) and np.isfinite(dd.intensity).all()
    last = (P - 1) // Pc * Pc
    picks = sorted({0, Pc - 1, Pc, 2 * Pc - 1, last - 1, last, P - 2, P - 1})
    ref = ps.MultisliceCalculator(progress=False, dtype="complex64")
    ref.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=[tuple(pp[i]) for i in picks])
    wf = npy(ref.run().wavefunction_data)[..., 0]
    want = block_sum((np.abs(wf.astype(np.complex128)) ** 2).mean(axis=1), 16, 16)
    err = np.abs(dd.intensity[picks] - want).max(axis=(-2, -1)) / want.max(axis=(-2, -1))
    print(f"P {P}, probe batch {Pc}: max diff / pattern max {err.max():.3e}")
    assert err.max() <= 1e-6, err
