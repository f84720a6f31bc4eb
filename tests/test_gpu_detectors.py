"""STEM detectors on the MI355X: msl_detect against numpy, run_detectors() against the reference golden, HAADFData, the oracle,
its own probe batching, and a scan whose (P, T, K) result could not exist on the device."""
import math
import time

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

KINDS = ("intensity", "amplitude", "com_x", "com_y")


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def _numpy_signals(W, bits, kinds, kx, ky):
    """W (..., wx, wy) complex -> (..., D) float64 sums and the (..., D) sums of |terms| (the scale of a signed CoM sum)"""
    I = np.abs(W.astype(np.complex128)) ** 2
    A = np.sqrt(I)
    KX = np.broadcast_to(kx.astype(np.float64)[:, None], I.shape[-2:])
    KY = np.broadcast_to(ky.astype(np.float64)[None, :], I.shape[-2:])
    out, scale = [], []
    for d, kind in enumerate(kinds):
        m = ((bits >> d) & 1).astype(np.float64)
        f = {"intensity": I, "amplitude": A, "com_x": KX * I, "com_y": KY * I}[kind]
        out.append((f * m).sum(axis=(-2, -1)))
        scale.append((np.abs(f) * m).sum(axis=(-2, -1)))
    return np.stack(out, -1), np.stack(scale, -1)


def _segment_detectors(n, rng):
    """n detectors of every kind: annuli, azimuthal segments (some wrapping through 0), a disc with the DC pixel"""
    from pyslice_amd import Detector
    dets = []
    for d in range(n):
        inner = [0.0, 2.0, 5.0, 10.0][d % 4]
        outer = [None, 40.0, 25.0, 80.0][(d // 4) % 4]
        az = None if d % 3 == 0 else tuple(float(v) for v in (rng.choice([0.0, 90.0, 200.0, 300.0]), rng.choice([45.0, 180.0, 270.0, 30.0])))
        if az is not None and az[0] == az[1]:
            az = None
        dets.append(Detector(f"d{d}", inner=inner, outer=outer, azimuth=az, signal=KINDS[d % 4]))
    return dets


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("B,T,shape,ld_pad,D", [(3, 5, (45, 63), 0, 16), (2, 4, (32, 32), 0, 1), (2, 3, (32, 32), 6, 5),
                                                (3, 2, (45, 63), 3, 3), (1, 2, (256, 256), 0, 8), (70, 1000, (4, 4), 0, 4),
                                                (2, 2, (6, 7), 1, 16)])
def test_detect_kernel_matches_numpy(ps, B, T, shape, ld_pad, D):
    """msl_detect on caller-held device memory: odd K, K % 4 == 0, ld > K (even: 16-byte loads; odd: scalar loads), more than
    65535 rows, 1 to 16 detectors of every signal kind with azimuthal segments; bitwise-equal repeats"""
    import torch
    from pyslice_amd import _native
    from pyslice_amd.stem_data import detector_bitmask
    rng = np.random.default_rng(B * 1000 + T + D)
    wx, wy = shape
    K, ld = wx * wy, wx * wy + ld_pad
    kx = np.fft.fftshift(np.fft.fftfreq(wx, 0.1)).astype(np.float32)
    ky = np.fft.fftshift(np.fft.fftfreq(wy, 0.1)).astype(np.float32)
    lam = 0.037
    dets = _segment_detectors(D, rng)
    bits = detector_bitmask(dets, kx, ky, lam)
    if B * T > 1000:                                       # tiny grid: random memberships, every pixel in some detector
        bits = rng.integers(0, 1 << D, size=(wx, wy)).astype(np.uint16)
    W = (rng.standard_normal((B, T, K)) + 1j * rng.standard_normal((B, T, K))).astype(np.complex64)
    W *= rng.choice([1e-3, 1.0, 30.0], size=(B, T, 1)).astype(np.float32)
    host = np.full((B, T, ld), np.nan + 1j * np.nan, dtype=np.complex64)      # pad pixels must never be read
    host[:, :, :K] = W
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    eng = _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, lam, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        kinds = [d.signal for d in dets]
        eng.set_detectors(bits.reshape(-1), kinds, kx, ky)
        src = (dW.data_ptr(), B, T, K, ld)
        got = eng.detect(src=src)
        want, scale = _numpy_signals(W.reshape(B, T, wx, wy), bits, kinds, kx, ky)
        assert got.shape == (B, T, D)
        err = np.abs(got - want) / np.maximum(scale, 1e-300)
        assert err.max() <= 1e-6, (err.max(), np.unravel_index(err.argmax(), err.shape))
        assert np.array_equal(eng.detect(src=src), got)                       # no atomics: bitwise reproducible
        if T > 2:
            assert np.array_equal(eng.detect(t0=1, count=2, src=src), got[:, 1:3])
        with pytest.raises(ValueError):
            eng.detect(src=(dW.data_ptr(), B, T, K - 1, ld))                   # the detectors cover K pixels
        with pytest.raises(ValueError):
            eng.detect(t0=T - 1, count=2, src=src)
    finally:
        eng.close()


def test_set_detectors_refusals(ps):
    from pyslice_amd import _native
    eng = _native.Engine(8, 8, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        k = np.zeros(8, dtype=np.float32)
        with pytest.raises(ValueError):
            eng.set_detectors(np.zeros(64), [], k, k)
        with pytest.raises(ValueError):
            eng.set_detectors(np.zeros(64), ["intensity"] * 17, k, k)
        with pytest.raises(ValueError):
            eng.set_detectors(np.zeros(64), [7], k, k)
        with pytest.raises(RuntimeError):
            eng.detect(src=(0, 1, 1, 64))                                        # no detectors set: MSL_ERR_STATE
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the reference golden and HAADFData
@pytest.mark.parametrize("probe_batch", [5, 6, 50])
def test_g9_haadf_through_detectors(ps, golden, probe_batch):
    g = golden("g9_haadf_32")
    pos = g["positions"]
    tr = ps.Trajectory(g["Z"], pos, np.zeros_like(pos), g["box"], 0.005)
    ca = float(g["collection_angle"])
    kw = dict(aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), probe_positions=g["probe_positions"])
    calc = ps.MultisliceCalculator(progress=False, detectors=[ps.Detector("adf", inner=ca, signal="amplitude")], probe_batch=probe_batch)
    calc.setup(tr, **kw)
    assert calc.probe_batch == min(probe_batch, 6)
    st = calc.run_detectors()
    assert st.signals.shape == (6, 2, 1)
    img = st.image("adf")
    assert img.shape == g["adf"].shape
    assert rel_l2(img, g["adf"]) < 1e-4
    ref = ps.MultisliceCalculator(progress=False)
    ref.setup(tr, **kw)
    wf = ref.run()
    wf.probe_positions = np.asarray(wf.probe_positions)
    assert rel_l2(img, ps.HAADFData(wf).calculateADF(collection_angle=ca)) <= 1e-6


# ------------------------------------------------------------------ 3. the oracle
def _stem_detectors(ps, aperture):
    D = ps.Detector
    return [D("bf", outer=aperture), D("abf", inner=aperture / 2, outer=aperture), D("adf", inner=aperture * 1.5, outer=150.0),
            D("dpc0", outer=aperture, azimuth=(0.0, 90.0)), D("dpc1", outer=aperture, azimuth=(90.0, 180.0)),
            D("dpc2", outer=aperture, azimuth=(180.0, 270.0)), D("dpc3", outer=aperture, azimuth=(270.0, 360.0)),
            D("comx", signal="com_x"), D("comy", outer=2 * aperture, signal="com_y"), D("haadf", inner=aperture * 1.5, signal="amplitude")]


@pytest.fixture(scope="module")
def oracle_case(ps):
    from oracle import multislice_oracle as orc
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, 3, ny=80, density=0.1, seed=11)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    rng = np.random.default_rng(12)
    pp = [tuple(v) for v in rng.random((20, 2)) * [lx, ly]]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp, workers=orc.usable_cores())
    return tr, pp, want["wavefunction_data"][..., 0]


@pytest.mark.parametrize("k_window,frame_batch,probe_batch", [(None, 1, 8), ((48, 40), 3, 20), ((33, 27), 2, 7)])
def test_detectors_match_oracle(ps, oracle_case, k_window, frame_batch, probe_batch):
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.stem_data import detector_bitmask
    tr, pp, wf = oracle_case
    dets = _stem_detectors(ps, 30.0)
    calc = ps.MultisliceCalculator(progress=False, detectors=dets, probe_batch=probe_batch, k_window=k_window, frame_batch=frame_batch)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert calc._engine.frame_batch == frame_batch
    st = calc.run_detectors()
    kx, ky = npy(st.kxs), npy(st.kys)
    nx, ny = wf.shape[-2:]
    if k_window is not None:
        x0, y0 = nx // 2 - k_window[0] // 2, ny // 2 - k_window[1] // 2
        wf = wf[..., x0:x0 + k_window[0], y0:y0 + k_window[1]]
    bits = detector_bitmask(dets, kx, ky, wavelength(100e3))
    want, _ = _numpy_signals(wf, bits, [d.signal for d in dets], kx, ky)
    total = (np.abs(wf) ** 2).sum(axis=(-2, -1)).max()
    kmax = max(np.abs(kx).max(), np.abs(ky).max())
    assert st.signals.shape == (20, 3, len(dets))
    for d, det in enumerate(dets):
        if det.signal.startswith("com"):
            assert np.abs(st.signals[..., d] - want[..., d]).max() <= 1e-4 * kmax * total, det.name
        else:
            assert rel_l2(st.signals[..., d], want[..., d]) <= 1e-4, det.name
    # the four DPC segments partition the BF disc
    assert rel_l2(st.signals[..., 3:7].sum(axis=-1), st.signals[..., 0]) < 1e-6


# ------------------------------------------------------------------ 4. probe batches do not change the result
def test_probe_batches_give_the_same_signals(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 5, 3, density=0.1, seed=21)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(22).random((19, 2)) * [lx, ly]]
    out = []
    for pb in (1, 7, 19):
        calc = ps.MultisliceCalculator(progress=False, detectors=_stem_detectors(ps, 25.0), probe_batch=pb, frame_batch=2)
        calc.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
        out.append(calc.run_detectors().signals)
    scale = np.abs(out[2]).max(axis=(0, 1), keepdims=True)
    for o in out[:2]:
        assert (np.abs(o - out[2]) / scale).max() <= 1e-6


# ------------------------------------------------------------------ 5. a scan larger than the device
def test_scan_larger_than_device_memory(ps):
    import torch
    from pyslice_amd import _native
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.stem_data import detector_bitmask
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(512, 4, 1, density=0.05, seed=31)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    K = len(xs) * len(ys)
    assert K == 512 * 512
    P = math.ceil(1.05 * torch.cuda.get_device_properties(0).total_memory / (K * 8))
    rng = np.random.default_rng(32)
    pp = rng.random((P, 2)) * [lx, ly]
    dets = _stem_detectors(ps, 30.0)[:8]
    calc = ps.MultisliceCalculator(progress=False, detectors=dets)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=[tuple(v) for v in pp])
    eng = calc._engine
    Pc, B = eng.n_probes, eng.frame_batch
    assert P > Pc
    assert eng.buffer_bytes(_native.BUF_WAVEFUNCTION) <= Pc * B * eng.result_pitch() * 8
    t0 = time.time()
    st = calc.run_detectors()
    assert time.time() - t0 < 120.0
    assert st.signals.shape == (P, 1, len(dets)) and np.isfinite(st.signals).all()
    last = (P - 1) // Pc * Pc
    picks = sorted({0, Pc - 1, Pc, 2 * Pc - 1, last - 1, last, P - 2, P - 1})
    ref = ps.MultisliceCalculator(progress=False, dtype="complex64")
    ref.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=[tuple(pp[i]) for i in picks])
    wf = npy(ref.run().wavefunction_data)[..., 0]
    kx, ky = npy(st.kxs), npy(st.kys)
    bits = detector_bitmask(dets, kx, ky, wavelength(100e3))
    want, scale = _numpy_signals(wf, bits, [d.signal for d in dets], kx, ky)
    err = np.abs(st.signals[picks] - want) / np.maximum(scale, 1e-300)
    assert err.max() <= 1e-6, err.max()
