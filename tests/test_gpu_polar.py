"""Polar detector on the MI355X: msl_polar_detect against polar_signals on caller-held memory, run_polar() against polar_signals
of the waves run() returns (probe and frame batching, k-windows, PRISM, frozen phonons), against run_detectors() in the same pass,
and a scan of 1600 positions."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

LAM = 0.037
NONE = 0xFFFF


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def _axes(shape):
    kx = np.fft.fftshift(np.fft.fftfreq(shape[0], 0.1)).astype(np.float32)
    ky = np.fft.fftshift(np.fft.fftfreq(shape[1], 0.1)).astype(np.float32)
    return kx, ky


# ------------------------------------------------------------------ 1. the kernel alone
# (B, T, shape, ld_pad, request: (step in mrad, R, A, rotation) or None for a random map over 4096 bins)
KERNEL_CASES = [(3, 5, (45, 63), 0, (10.0, 20, 1, 0.0)),
                (2, 3, (32, 32), 6, (30.0, 7, 12, 15.0)),
                (3, 2, (45, 63), 3, (40.0, 5, 3, 0.0)),
                (1, 2, (256, 256), 0, (3.0, 64, 16, 0.0)),
                (2, 2, (6, 7), 1, (100.0, 2, 1, 0.0)),
                (70, 1000, (4, 4), 0, None)]


@pytest.mark.parametrize("B,T,shape,ld_pad,req", KERNEL_CASES)
def test_polar_kernel_matches_numpy(ps, B, T, shape, ld_pad, req):
    """msl_polar_detect on caller-held device memory: odd K, ld > K (pad pixels hold NaN: never read), bins shorter and longer than
    a wave, empty bins (exactly 0), 4096 bins over more than 65535 rows; bitwise-equal repeats; a frame range; the refusals"""
    import torch
    from pyslice_amd import PolarDetector, _native, polar_bins, polar_signals
    from pyslice_amd.polar_data import bin_counts
    rng = np.random.default_rng(B * 1000 + T + shape[0])
    wx, wy = shape
    K, ld = wx * wy, wx * wy + ld_pad
    if req is None:
        n_bins = 4096
        bins = rng.integers(0, n_bins, size=(wx, wy)).astype(np.uint16)
        bins[rng.random((wx, wy)) < 0.25] = NONE
        bins[0, 0], bins[1, 2] = n_bins - 1, 0                       # the first and the last bin are in use
    else:
        step, R, A, rot = req
        pol = PolarDetector(outer=step * R, step=step, n_azimuthal=A, rotation=rot)
        assert (pol.n_rings, pol.n_azimuthal) == (R, A)
        n_bins = pol.n_bins
        bins = polar_bins(pol, *_axes(shape), LAM)
    counts = bin_counts(bins, n_bins)
    assert counts.sum() > 0
    if shape == (256, 256):
        assert (counts.reshape(64, 16).sum(axis=1) > 64).mean() > 0.5 and counts.max() > 64 > counts[counts > 0].min()
    W = (rng.standard_normal((B, T, K)) + 1j * rng.standard_normal((B, T, K))).astype(np.complex64)
    W *= rng.choice([1e-3, 1.0, 30.0], size=(B, T, 1)).astype(np.float32)
    host = np.full((B, T, ld), np.nan + 1j * np.nan, dtype=np.complex64)      # pad pixels must never be read
    host[:, :, :K] = W
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    eng = _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, LAM, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        src = (dW.data_ptr(), B, T, K, ld)
        with pytest.raises(RuntimeError):
            eng.polar_detect(src=src)                                  # no bin map yet: MSL_ERR_STATE
        eng.set_polar(bins.reshape(-1), n_bins)
        got = eng.polar_detect(src=src)
        assert got.shape == (B, T, n_bins)
        want = polar_signals(W.reshape(B, T, wx, wy), bins, n_bins)
        used = np.flatnonzero(counts)                                  # (column subsets: the 4096-bin case is 2.3 GB per array)
        g, w = got[..., used], want[..., used]
        err = np.abs(g - w) / np.maximum(w, np.finfo(np.float64).tiny)
        print(f"B={B} T={T} {wx}x{wy} ld+{ld_pad} bins={n_bins}: worst relative error {err.max():.3e}")
        assert err.max() <= 1e-6, (err.max(), np.unravel_index(err.argmax(), err.shape))
        assert np.count_nonzero(got) == np.count_nonzero(g)            # empty bins are exactly 0
        assert np.array_equal(eng.polar_detect(src=src), got)          # no atomics: bitwise reproducible
        if T > 2:
            assert np.array_equal(eng.polar_detect(t0=1, count=2, src=src), got[:, 1:3])
        else:
            assert np.array_equal(eng.polar_detect(t0=1, count=1, src=src), got[:, 1:2])
        with pytest.raises(ValueError):
            eng.polar_detect(src=(dW.data_ptr(), B, T, K - 1, ld))     # the bin map covers K pixels
        with pytest.raises(ValueError):
            eng.polar_detect(t0=T - 1, count=2, src=src)
    finally:
        eng.close()


def test_set_polar_refusals(ps):
    from pyslice_amd import _native
    eng = _native.Engine(8, 8, 1, 0.1, 0.1, 1.0, LAM, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        with pytest.raises(ValueError):
            eng.set_polar(np.zeros(63, dtype=np.uint16), 4)
        with pytest.raises(ValueError):
            eng.set_polar(np.zeros(64, dtype=np.uint16), 0)
        with pytest.raises(ValueError):
            eng.set_polar(np.zeros(64, dtype=np.uint16), 4097)
        with pytest.raises(ValueError):
            eng.set_polar(np.full(64, 4, dtype=np.uint16), 4)          # a bin id equal to n_bins
        with pytest.raises(RuntimeError):
            eng.polar_detect(src=(0, 1, 1, 64))                        # the refused maps left none set
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. through the calculator
def _request(ps, **kw):
    return ps.PolarDetector(outer=60.0, step=2.0, n_azimuthal=4, **{"per_frame": True, **kw})


@pytest.fixture(scope="module")
def case(ps):
    """the trajectory and probes of test_gpu_detectors' oracle case, and a cache of what the tests below share: the waves of
    run() per set-up and the per-frame polar result per (k_window, frame_batch, probe_batch)"""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, 3, ny=80, density=0.1, seed=11)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(12).random((20, 2)) * [lx, ly]]
    waves, polar = {}, {}

    def run_waves(source=None, **kw):
        key = (id(source), tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in waves:
            calc = ps.MultisliceCalculator(progress=False, **kw)
            calc.setup(tr if source is None else source, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
            wf = calc.run()
            waves[key] = (npy(wf.wavefunction_data)[..., 0], npy(wf.kxs), npy(wf.kys))
        return waves[key]

    def run_polar(request, source=None, **kw):
        calc = ps.MultisliceCalculator(progress=False, polar=request, **kw)
        calc.setup(tr if source is None else source, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        return calc, calc.run_polar()
    return dict(tr=tr, pp=pp, run_waves=run_waves, run_polar=run_polar, polar=polar)


def _want(ps, request, waves):
    from pyslice_amd.multislice import wavelength
    wf, kx, ky = waves
    bins = ps.polar_bins(request, kx, ky, wavelength(100e3))
    return ps.polar_signals(wf, bins, request.n_bins).reshape(wf.shape[:2] + (request.n_rings, request.n_azimuthal)), bins


CONFIGS = [(None, 1, 8), ((48, 40), 3, 20), ((33, 27), 2, 7)]


@pytest.mark.parametrize("k_window,frame_batch,probe_batch", CONFIGS)
def test_run_polar_matches_the_waves_of_run(ps, case, k_window, frame_batch, probe_batch):
    from pyslice_amd.polar_data import bin_counts
    req = _request(ps)
    calc, res = case["run_polar"](req, k_window=k_window, frame_batch=frame_batch, probe_batch=probe_batch)
    assert calc._engine.frame_batch == frame_batch and calc.probe_batch == probe_batch
    case["polar"][(k_window, frame_batch, probe_batch)] = res
    want, bins = _want(ps, req, case["run_waves"](k_window=k_window))
    assert res.signals.shape == (20, 3, 30, 4) and res.stem is None
    assert np.array_equal(res.counts, bin_counts(bins, req.n_bins).reshape(30, 4)) and np.array_equal(res.edges, np.arange(0.0, 61.0, 2.0))
    err = rel_l2(res.signals, want)
    print(f"run_polar k_window={k_window} frame_batch={frame_batch} probe_batch={probe_batch}: rel-L2 {err:.3e}")
    assert err <= 1e-6
    assert not res.signals[..., res.counts == 0].any()


@pytest.mark.parametrize("k_window,frame_batch,probe_batch", CONFIGS[1:])
def test_frame_mean_is_the_mean_of_the_frames(ps, case, k_window, frame_batch, probe_batch):
    key = (k_window, frame_batch, probe_batch)
    per_frame = case["polar"].get(key) or case["run_polar"](_request(ps), k_window=k_window, frame_batch=frame_batch, probe_batch=probe_batch)[1]
    _, res = case["run_polar"](_request(ps, per_frame=False), k_window=k_window, frame_batch=frame_batch, probe_batch=probe_batch)
    assert res.signals.shape == (20, 30, 4)
    assert np.allclose(res.signals, per_frame.signals.mean(axis=1), rtol=1e-12, atol=0)


def test_detectors_in_the_same_pass(ps, case):
    """.stem is bitwise what run_detectors() gives alone; the same detectors chosen after the run, from the bins"""
    D = ps.Detector
    dets = [D("bf", outer=30.0), D("adf", inner=40.0, outer=60.0)] + [D(f"q{a}", outer=30.0, azimuth=(90.0 * a, 90.0 * a + 90.0)) for a in range(4)]
    kw = dict(k_window=(48, 40), frame_batch=3, probe_batch=7)
    _, res = case["run_polar"](_request(ps), detectors=dets, **kw)
    alone = ps.MultisliceCalculator(progress=False, detectors=dets, **kw)
    alone.setup(case["tr"], aperture=30.0, voltage_eV=100e3, probe_positions=case["pp"])
    st = alone.run_detectors()
    assert res.stem is not None and np.array_equal(res.stem.signals, st.signals)
    assert [d.name for d in res.stem.detectors] == [d.name for d in dets]
    after = res.to_stem(dets)
    assert after.signals.shape == st.signals.shape == (20, 3, 6)
    for d, det in enumerate(dets):
        got = res.integrate(det.inner, det.outer, det.azimuth)
        assert np.array_equal(got, after.signals[..., d])
        err = np.abs(got - st.signals[..., d]) / st.signals[..., d]
        print(f"{det.name}: bins against msl_detect, worst relative difference {err.max():.3e}")
        assert err.max() <= 1e-6, det.name
    assert np.allclose(after.image("adf"), st.image("adf"), rtol=1e-6, atol=0)


def test_all_bins_add_up_to_the_whole_pattern(ps, case):
    """full grid, outer edge past the corner of the spectrum (262 mrad): no intensity is lost or counted twice"""
    req = ps.PolarDetector(outer=280.0, step=10.0, n_azimuthal=4, per_frame=True)
    _, res = case["run_polar"](req, detectors=[ps.Detector("all")], frame_batch=3, probe_batch=20)
    assert res.counts.sum() == 96 * 80
    total, whole = res.signals.sum(axis=(-2, -1)), res.stem.signals[..., 0]
    err = np.abs(total - whole) / whole
    print(f"conservation: worst relative difference {err.max():.3e}")
    assert err.max() <= 1e-6


def test_run_polar_with_prism(ps, case):
    from pyslice_amd.prism import Prism
    req = _request(ps)
    _, res = case["run_polar"](req, prism=Prism(1), probe_batch=7)
    want, _ = _want(ps, req, case["run_waves"](prism=Prism(1)))
    err = rel_l2(res.signals, want)
    print(f"run_polar with Prism(1): rel-L2 {err:.3e}")
    assert res.signals.shape == (20, 3, 30, 4) and err <= 1e-6


def test_run_polar_with_frozen_phonons(ps, case):
    tr = case["tr"]
    fp = ps.FrozenPhonons(tr.atom_types, tr.positions[0], tr.box_matrix, 0.05, n_configs=2, seed=3)
    req = _request(ps)
    _, res = case["run_polar"](req, source=fp, frame_batch=2, probe_batch=8)
    want, _ = _want(ps, req, case["run_waves"](source=fp, frame_batch=2))
    err = rel_l2(res.signals, want)
    print(f"run_polar with FrozenPhonons: rel-L2 {err:.3e}")
    assert res.signals.shape == (20, 2, 30, 4) and err <= 1e-6
    assert rel_l2(res.signals[:, 0], res.signals[:, 1]) > 1e-3         # two different configurations


# ------------------------------------------------------------------ 3. a scan
def test_scan_of_1600_positions(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 6, 1, density=0.1, seed=21)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    assert (len(xs), len(ys)) == (64, 64)
    pp = [(x, y) for x in np.linspace(0.0, lx, 40, endpoint=False) for y in np.linspace(0.0, ly, 40, endpoint=False)]
    req = ps.PolarDetector(outer=120.0, step=10.0, n_azimuthal=4)
    calc = ps.MultisliceCalculator(progress=False, polar=req, probe_batch=256)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert calc.probe_batch == 256
    res = calc.run_polar()
    assert res.signals.shape == (1600, 12, 4) and np.isfinite(res.signals).all()
    ref = ps.MultisliceCalculator(progress=False, detectors=[ps.Detector("bf", outer=30.0)], probe_batch=256)
    ref.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    want = ref.run_detectors().image("bf")
    got = res.image(0.0, 30.0)
    assert got.shape == want.shape == (40, 40)
    err = np.abs(got - want) / want
    print(f"BF image of the scan: worst relative difference {err.max():.3e}")
    assert err.max() <= 1e-6
