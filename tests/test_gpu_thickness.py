"""Thickness series of the probe-batch modes on the MI355X (MultisliceCalculator(thickness=...), msl_set_layer_reduce).

Every tapped layer is reduced inside the launch sequence of the slice loop, out of ONE reused block, with the launches of
msl_detect / msl_polar_detect / msl_diffract.  So the numbers must be, bit for bit, what those calls give on the blocks of
msl_set_layers (1), and within the bound of each kernel's own test what NumPy gives on the waves of run(layers=...) (2); the last
entry is the run without a thickness series (3); the pacbed accumulator is the probe mean of the patterns (4); device memory does
not grow with the number of entries beyond the staging (5); the two layer modes exclude each other and clear cleanly (6).

Grids: 64 x 64 and 96 x 80 run the convolution passes (scheme B: every pass transposes), 256 x 256 is the smallest grid of scheme A
(nz - 1 - k of the entries [0, 1, nz - 2] has both parities at nz = 5 and 6), 600 x 500 the mixed-radix passes; the two-pass loop
(fft_path = 1) at 96 x 80, the smallest grid tests/test_gpu_layers.py runs it on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EV, MRAD = 100e3, 30.0
P, T, PROBE_BATCH, FRAME_BATCH = 5, 3, 2, 2
BIN = (4, 4)


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def _detectors():
    from pyslice_amd import Detector
    return [Detector("bf", outer=20.0), Detector("adf", inner=40.0, outer=150.0, signal="amplitude"),
            Detector("comx", outer=35.0, signal="com_x")]


def _polar(per_frame=True):
    from pyslice_amd import PolarDetector
    return PolarDetector(outer=60.0, step=20.0, n_azimuthal=4, rotation=10.0, per_frame=per_frame)


def _trajectory(nx, ny, nz, frames=T):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(nx, nz, frames, ny=ny, density=0.05, seed=nx + 7 * ny + nz)


def _probes(tr, n):
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    return [tuple(v) for v in np.random.default_rng(11).random((n, 2)) * [lx, ly]]


def _block_sum(I, bx, by):
    wx, wy = I.shape[-2:]
    return I.reshape(I.shape[:-2] + (wx // bx, bx, wy // by, by)).sum(axis=(-3, -1))


# ------------------------------------------------------------------ 1. bit for bit the existing calls on the blocks of msl_set_layers
ENGINE_CASES = [
    # nx, ny, nz, fft_path, k_window
    (64, 64, 5, 0, None), (64, 64, 6, 0, None), (256, 256, 5, 0, None), (256, 256, 6, 0, None), (600, 500, 5, 0, None),
    (96, 80, 5, 0, None), (96, 80, 5, 1, None), (64, 64, 5, 0, (16, 16)),
]


def _engine(nx, ny, nz, fft_path, window, n_probes=2, n_frames=2):
    """engine of 2 probes x 2 frame slots at a frame batch of 2 with its potentials built, detectors and bin map set"""
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.polar_data import polar_bins
    from pyslice_amd.potentials import gridFromTrajectory, loadKirkland, slice_edges
    from pyslice_amd.stem_data import detector_bitmask
    tr = _trajectory(nx, ny, nz, frames=2)
    xs, ys, zs, *_ = gridFromTrajectory(tr, sampling=0.1, slice_thickness=0.5)
    assert (len(xs), len(ys), len(zs)) == (nx, ny, nz)
    eng = _native.Engine(nx, ny, nz, xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(EV), interaction_sigma(EV),
                         n_probes=n_probes, n_frames=n_frames, fft_path=fft_path, window=window, frame_batch=2)
    eng.set_kirkland(loadKirkland())
    eng.set_slices(*slice_edges(np.asarray(zs, dtype=np.float64)))
    kx = np.fft.fftshift(np.fft.fftfreq(nx, 0.1)).astype(np.float32)
    ky = np.fft.fftshift(np.fft.fftfreq(ny, 0.1)).astype(np.float32)
    if window:
        kx, ky = kx[nx // 2 - window[0] // 2:][:window[0]], ky[ny // 2 - window[1] // 2:][:window[1]]
    dets, pol = _detectors(), _polar()
    eng.set_detectors(detector_bitmask(dets, kx, ky, wavelength(EV)).reshape(-1), [d.signal for d in dets], kx, ky)
    eng.set_polar(polar_bins(pol, kx, ky, wavelength(EV)).reshape(-1), pol.n_bins)
    eng.build_potentials(tr.positions[:2], np.asarray(tr.atom_types, dtype=np.int32), 2)
    eng.set_probes(MRAD, np.asarray(_probes(tr, n_probes), dtype=np.float64))
    return eng


def _plain_exit(eng):
    return eng.detect(0, 2), eng.polar_detect(0, 2), eng.diffract(0, 2, bin=BIN)


@pytest.mark.parametrize("nx,ny,nz,fft_path,window", ENGINE_CASES)
def test_same_numbers_as_the_calls_on_the_layer_blocks(ps, nx, ny, nz, fft_path, window):
    from pyslice_amd import _native
    slices = [0, 1, nz - 2]
    L = len(slices) + 1
    eng = _engine(nx, ny, nz, fft_path, window)
    try:
        # the existing path: full blocks, one call per block and signal
        eng.set_layers(slices)
        eng.propagate_frames(0, 2)
        eng.synchronize()
        pitch, K = eng.result_pitch(_native.BUF_LAYERS), eng.wx * eng.wy
        base, block = eng.device_ptr(_native.BUF_LAYERS), 2 * 2 * pitch * 8
        want = {B: [] for B in (1, 2)}
        for l in range(L):
            for B in (1, 2):
                src = (base + l * block, B, 2, K, pitch)
                want[B].append((eng.detect(0, 2, src=src), eng.polar_detect(0, 2, src=src),
                                eng.diffract(0, 2, bin=BIN, src=(base + l * block, B, 2, eng.wx, eng.wy, pitch))))
        eng.set_layers([])
        # the thickness series: one block, reduced in the sequence, one fetch
        what = _native.LR_DETECT | _native.LR_POLAR | _native.LR_DIFFRACT
        eng.set_layer_reduce(slices, what, bin=BIN)
        assert eng.buffer_bytes(_native.BUF_LAYERS) == eng.buffer_bytes(_native.BUF_WAVEFUNCTION)      # no second layer block
        eng.propagate_frames(0, 2)
        for B in (2, 1):                                             # (1: what a padded probe batch fetches)
            det, pol, pat = eng.layer_fetch(2, B=B)
            assert det.shape == (L, B, 2, 3) and pol.shape == (L, B, 2, 12) and pat.shape == (L, B, eng.wx // 4, eng.wy // 4)
            for l in range(L):
                assert np.array_equal(det[l], want[B][l][0]), (l, "detect")
                assert np.array_equal(pol[l], want[B][l][1]), (l, "polar")
                assert np.array_equal(pat[l], want[B][l][2]), (l, "diffract")
            assert det[-1].any() and pol[-1].any() and pat[-1].all() and not np.array_equal(det[0], det[-1])
        # the exit block is still the wavefunction buffer of every other call
        plain = _plain_exit(eng)
        assert all(np.array_equal(a, b) for a, b in zip(plain, want[2][-1]))
        with pytest.raises(ValueError):
            eng.layer_fetch(1)                                       # the last sequence ran 2 frames
    finally:
        eng.close()


def test_single_frame_sequence_and_pacbed_accumulator(ps):
    """msl_propagate_frame (a frame batch of 1 takes it) reduces one frame slot; the accumulator is the probe sum of the fetched
    patterns to 1e-12 (the order of float64 additions of non-negative terms is the same here: probe order) and repeats bitwise"""
    from pyslice_amd import _native
    eng = _engine(64, 64, 5, 0, None, n_probes=3)
    try:
        eng.set_layer_reduce([1, 3], _native.LR_DIFFRACT | _native.LR_PACBED | _native.LR_DETECT, bin=BIN)
        eng.propagate_frame(1)
        det, pol, pat = eng.layer_fetch(1)
        assert det.shape == (3, 3, 1, 3) and pol is None and pat.shape == (3, 3, 16, 16)
        assert np.array_equal(det[-1], eng.detect(1, 1)) and np.array_equal(pat[-1], eng.diffract(1, 1, bin=BIN))
        accs = []
        for _ in range(2):
            eng.layer_pacbed_reset()
            eng.layer_pacbed_add(2)
            eng.layer_pacbed_add(3)
            accs.append(eng.layer_pacbed())
        want = pat[:, :2].sum(axis=1) + pat.sum(axis=1)
        assert np.allclose(accs[0], want, rtol=1e-12, atol=0) and np.array_equal(accs[0], accs[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. / 3. the calculator against the definition and its own plain run
CALC_CASES = [(64, 64, 5, None), (64, 64, 6, None), (256, 256, 5, None), (256, 256, 6, None), (600, 500, 5, None), (96, 80, 5, None),
              (64, 64, 5, (16, 16))]


@pytest.fixture(scope="module")
def runs(ps):
    """per case, computed once and left unchanged: the waves of run(layers=...), the thickness runs and the plain runs"""
    from pyslice_amd import Diffraction
    cache = {}

    def get(nx, ny, nz, window):
        key = (nx, ny, nz, window)
        if key in cache:
            return cache[key]
        tr = _trajectory(nx, ny, nz)
        pp = _probes(tr, P)
        entries = [0, 1, nz - 2]

        def calc(**kw):
            c = ps.MultisliceCalculator(progress=False, k_window=window, **kw)
            c.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
            assert (c.nx, c.ny, c.nz) == (nx, ny, nz)
            return c
        batched = dict(probe_batch=PROBE_BATCH, frame_batch=FRAME_BATCH)
        wf = calc(layers=entries, dtype="complex64").run()
        out = dict(entries=entries + [nz - 1], W=npy(wf.wavefunction_data), kxs=npy(wf.kxs), kys=npy(wf.kys),
                   polar=calc(polar=_polar(), detectors=_detectors(), thickness=entries, **batched).run_polar(),
                   polar_plain=calc(polar=_polar(), detectors=_detectors(), **batched).run_polar(),
                   diff=calc(diffraction=Diffraction(bin=BIN), detectors=_detectors(), thickness=entries, **batched).run_diffraction(),
                   diff_plain=calc(diffraction=Diffraction(bin=BIN), detectors=_detectors(), **batched).run_diffraction(),
                   stem=calc(detectors=_detectors(), thickness=entries, **batched).run_detectors(),
                   stem_plain=calc(detectors=_detectors(), **batched).run_detectors())
        assert out["W"].shape[:2] == (P, T) and out["W"].shape[-1] == 4
        cache[key] = out
        return out
    return get


@pytest.mark.parametrize("nx,ny,nz,window", CALC_CASES)
def test_signals_match_the_definition_on_the_layer_waves(ps, runs, nx, ny, nz, window):
    """NumPy float64 on the (P, T, wx, wy, L) waves of run(layers=...): Detector.member masks held to 1e-6 of the sum of |terms|
    (tests/test_gpu_detectors.py), polar_signals to 1e-6 of each non-empty bin (tests/test_gpu_polar.py), the bx x by intensity sums to
    1e-6 of each bin (tests/test_gpu_diffraction.py)"""
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.polar_data import polar_bins, polar_signals
    r = runs(nx, ny, nz, window)
    W, kx, ky, lam = r["W"].astype(np.complex128), r["kxs"], r["kys"], wavelength(EV)
    L = W.shape[-1]
    assert list(r["polar"].layer) == r["entries"] and list(r["diff"].layer) == r["entries"] and list(r["stem"].layer) == r["entries"]
    assert np.all(np.diff(r["stem"].thickness) > 0) and abs(r["stem"].thickness[-1] - nz * 0.5) < 0.26
    I = np.abs(np.moveaxis(W, -1, 0)) ** 2                              # (L, P, T, wx, wy)
    # detectors, from all three passes
    KX, KY = kx.astype(np.float64)[:, None], ky.astype(np.float64)[None, :]
    for d, det in enumerate(_detectors()):
        m = det.member(kx, ky, lam).astype(np.float64)
        f = {"intensity": I, "amplitude": np.sqrt(I), "com_x": KX * I, "com_y": KY * I}[det.signal]
        want, scale = (f * m).sum(axis=(-2, -1)), (np.abs(f) * m).sum(axis=(-2, -1))
        assert scale.min() > 0
        for name in ("stem", "polar", "diff"):
            st = r[name] if name == "stem" else r[name].stem
            assert st.signals.shape == (P, T, 3, L)
            err = np.abs(np.moveaxis(st.signals[:, :, d], -1, 0) - want) / scale
            print(f"{nx}x{ny} nz={nz} {name} detector {det.name}: worst error / scale {err.max():.3e}")
            assert err.max() <= 1e-6, (name, det.name, err.max())
    # polar bins
    pol = _polar()
    bins = polar_bins(pol, kx, ky, lam)
    want = np.moveaxis(polar_signals(np.moveaxis(W, -1, 0), bins, pol.n_bins), 0, -1).reshape(P, T, 3, 4, L)
    used = want > 0
    assert r["polar"].signals.shape == (P, T, 3, 4, L) and used.any() and not r["polar"].signals[~used].any()
    err = np.abs(r["polar"].signals[used] - want[used]) / want[used]
    print(f"{nx}x{ny} nz={nz} polar: worst relative error {err.max():.3e}")
    assert err.max() <= 1e-6
    # patterns: the frame mean of the bx x by intensity sums
    want = np.moveaxis(_block_sum(I.mean(axis=2), *BIN), 0, -1)
    assert r["diff"].intensity.shape == want.shape == (P, W.shape[2] // 4, W.shape[3] // 4, L)
    err = np.abs(r["diff"].intensity - want) / want
    print(f"{nx}x{ny} nz={nz} patterns: worst relative error {err.max():.3e}")
    assert err.max() <= 1e-6
    # the thicknesses differ: a series that repeated one layer would not
    assert not np.array_equal(r["diff"].intensity[..., 0], r["diff"].intensity[..., -1])


@pytest.mark.parametrize("nx,ny,nz,window", CALC_CASES)
def test_last_entry_is_the_run_without_thickness(ps, runs, nx, ny, nz, window):
    r = runs(nx, ny, nz, window)
    assert np.array_equal(r["stem"].at(-1).signals, r["stem_plain"].signals)
    assert np.array_equal(r["polar"].at(-1).signals, r["polar_plain"].signals)
    assert np.array_equal(r["polar"].at(-1).stem.signals, r["polar_plain"].stem.signals)
    assert np.array_equal(r["diff"].at(-1).intensity, r["diff_plain"].intensity)
    assert np.array_equal(r["diff"].at(-1).stem.signals, r["diff_plain"].stem.signals)
    assert type(r["polar"].at(-1)) is type(r["polar_plain"]) and r["polar"].at(-1).layer is None
    assert np.array_equal(r["polar"].image(0.0, 40.0), r["polar_plain"].image(0.0, 40.0))
    assert np.array_equal(r["diff"].pacbed(), r["diff_plain"].pacbed())


def test_frame_mean_polar_and_phonon_source(ps):
    """per_frame=False sums the frames of every entry; a FrozenPhonons source goes through the same pass"""
    from pyslice_amd import FrozenPhonons
    tr = _trajectory(64, 64, 5)
    src = FrozenPhonons.from_trajectory(tr, sigma=0.08, n_configs=T, seed=5)
    pp = _probes(tr, P)
    out = {}
    for per_frame in (True, False):
        c = ps.MultisliceCalculator(progress=False, polar=_polar(per_frame), thickness=[0, 3], probe_batch=PROBE_BATCH, frame_batch=FRAME_BATCH)
        c.setup(src, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
        out[per_frame] = c.run_polar()
    assert out[False].signals.shape == (P, 3, 4, 3) and out[True].signals.shape == (P, T, 3, 4, 3)
    assert np.allclose(out[False].signals, out[True].signals.mean(axis=1), rtol=1e-12, atol=0)


# ------------------------------------------------------------------ 4. patterns="pacbed"
@pytest.mark.parametrize("nx,ny,nz,window", [(64, 64, 6, None), (96, 80, 5, None)])
def test_pacbed_is_the_probe_mean_and_repeats_bitwise(ps, runs, nx, ny, nz, window):
    """the accumulator adds the probes in order and the host adds the frame batches; the position run adds the frame batches per
    probe and means over the probes afterwards: float64 sums of non-negative terms in another order, P * 2^-53 apart at most,
    far inside 1e-12"""
    from pyslice_amd import Diffraction
    from pyslice_amd.thickness import Thickness
    r = runs(nx, ny, nz, window)
    tr = _trajectory(nx, ny, nz)
    got = []
    for _ in range(2):
        c = ps.MultisliceCalculator(progress=False, diffraction=Diffraction(bin=BIN), thickness=Thickness(slices=[0, 1, nz - 2], patterns="pacbed"),
                                    probe_batch=PROBE_BATCH, frame_batch=FRAME_BATCH)
        c.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=_probes(tr, P))
        got.append(c.run_diffraction())
    assert got[0].intensity.shape == (nx // 4, ny // 4, 4) and got[0].patterns == "pacbed"
    assert np.allclose(got[0].intensity, r["diff"].intensity.mean(axis=0), rtol=1e-12, atol=0)
    assert np.array_equal(got[0].intensity, got[1].intensity)
    assert np.array_equal(got[0].pacbed(), got[0].intensity[..., -1])


# ------------------------------------------------------------------ 5. memory
def test_memory_is_one_block_and_the_staging_arithmetic(ps):
    from pyslice_amd import _native
    nx, ny, nz = 64, 64, 6
    eng = _engine(nx, ny, nz, 0, None)
    try:
        Pn, Tn, D, nb, M = 2, 2, 3, 12, (nx // 4) * (ny // 4)
        block = eng.buffer_bytes(_native.BUF_WAVEFUNCTION)
        assert block == Pn * Tn * eng.result_pitch() * 8
        assert eng.layer_reduce_bytes(_native.LR_BYTES_STAGING) == 0
        got = {}
        for slices in ([0], [0, 1, 2, 3]):                           # 2 and 5 thickness entries
            L = len(slices) + 1
            eng.set_layer_reduce(slices, _native.LR_DETECT | _native.LR_POLAR | _native.LR_DIFFRACT | _native.LR_PACBED, bin=BIN)
            got[L] = [eng.layer_reduce_bytes(w) for w in (_native.LR_BYTES_BLOCK, _native.LR_BYTES_TAP, _native.LR_BYTES_STAGING)]
            assert got[L][2] == 8 * L * (Pn * Tn * D + Pn * Tn * nb + Pn * M + M)
            assert got[L][0] == block and eng.buffer_bytes(_native.BUF_LAYERS) == block
        assert got[2][:2] == got[5][:2]                              # the block and the tap buffer do not grow with the entries
        assert got[5][2] - got[2][2] == 8 * 3 * (Pn * Tn * D + Pn * Tn * nb + Pn * M + M)
        eng.set_layer_reduce([0, 3], _native.LR_DETECT)
        assert eng.layer_reduce_bytes(_native.LR_BYTES_STAGING) == 8 * 3 * Pn * Tn * D
        eng.set_layer_reduce([], 0)
        assert [eng.layer_reduce_bytes(w) for w in range(3)] == [0, 0, 0]
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. mode hygiene
def test_modes_exclude_each_other_and_clear(ps):
    import torch
    from pyslice_amd import _native
    nx, ny, nz = 64, 64, 5
    fresh = _engine(nx, ny, nz, 0, None)
    try:
        fresh.propagate_frames(0, 2)
        want = _plain_exit(fresh)
    finally:
        fresh.close()
    eng = _engine(nx, ny, nz, 0, None)
    try:
        with pytest.raises(RuntimeError):
            eng.layer_fetch(2)                                       # no mode
        eng.set_layer_reduce([0, 2], _native.LR_DETECT)
        with pytest.raises(RuntimeError):
            eng._chk(eng._lib.msl_layer_fetch(eng._h, 2, 2, None, None, None))      # MSL_ERR_STATE before the first sequence
        with pytest.raises(RuntimeError):
            eng.set_layers([1])                                      # MSL_ERR_STATE while the reduce mode is on
        with pytest.raises(ValueError):
            eng.set_layer_reduce([2, 1], _native.LR_DETECT)          # not increasing
        with pytest.raises(ValueError):
            eng.set_layer_reduce([nz - 1], _native.LR_DETECT)        # the exit is always the last layer
        with pytest.raises(ValueError):
            eng.set_layer_reduce([1], 16)
        with pytest.raises(ValueError):
            eng.set_layer_reduce([1], _native.LR_DIFFRACT, bin=(5, 4))
        assert eng.reduce_layers == [0, 2]                           # (a refused call leaves the mode, and its Python mirror, on)
        # the staging has rows of 3 detectors: another count is MSL_ERR_STATE while the mode is on, other masks of 3 are fine
        from pyslice_amd import Detector, PolarDetector
        from pyslice_amd.multislice import wavelength
        from pyslice_amd.polar_data import polar_bins
        from pyslice_amd.stem_data import detector_bitmask
        k = np.fft.fftshift(np.fft.fftfreq(64, 0.1)).astype(np.float32)

        def set_detectors(dets):
            eng.set_detectors(detector_bitmask(dets, k, k, wavelength(EV)).reshape(-1), [d.signal for d in dets], k, k)
        with pytest.raises(RuntimeError):
            set_detectors(_detectors() + [Detector("more", outer=50.0)])
        with pytest.raises(RuntimeError):
            set_detectors(_detectors()[:2])
        set_detectors(_detectors())
        other = PolarDetector(outer=60.0, step=10.0)
        eng.set_polar(polar_bins(other, k, k, wavelength(EV)).reshape(-1), other.n_bins)      # (the polar bit is off: any map)
        eng.set_layer_reduce([0, 2], _native.LR_DETECT | _native.LR_POLAR)
        with pytest.raises(RuntimeError):
            eng.set_polar(polar_bins(_polar(), k, k, wavelength(EV)).reshape(-1), _polar().n_bins)   # 12 bins, the staging has 6
        eng.set_layer_reduce([0, 2], _native.LR_DETECT)
        eng.set_polar(polar_bins(_polar(), k, k, wavelength(EV)).reshape(-1), _polar().n_bins)
        eng.propagate_frames(0, 2)
        det, pol, pat = eng.layer_fetch(2)
        assert pol is None and pat is None and np.array_equal(det[-1], want[0])
        eng.set_layer_reduce([], 0)
        eng.set_layers([1])
        with pytest.raises(RuntimeError):
            eng.set_layer_reduce([0], _native.LR_DETECT)             # and the reverse order
        eng.set_layers([])
        # cleared: a plain run whose exit signals are a fresh handle's
        eng.propagate_frames(0, 2)
        assert all(np.array_equal(a, b) for a, b in zip(_plain_exit(eng), want))
    finally:
        eng.close()
    # a handle without detectors or a bin map: MSL_ERR_STATE
    from pyslice_amd.multislice import interaction_sigma, wavelength
    bare = _native.Engine(64, 64, 4, 0.1, 0.1, 0.5, wavelength(EV), interaction_sigma(EV), n_probes=1, n_frames=1)
    try:
        for what in (_native.LR_DETECT, _native.LR_POLAR):
            with pytest.raises(RuntimeError):
                bare.set_layer_reduce([1], what)
        bare.set_layer_reduce([1], _native.LR_DIFFRACT, bin=(2, 2))
    finally:
        bare.close()
    # destroying a handle with the mode on leaves nothing behind: the third cycle ends where the first did
    import gc

    def cycle():
        eng = _engine(256, 256, 5, 0, None)
        eng.set_layer_reduce([0, 1, 3], _native.LR_DETECT | _native.LR_POLAR | _native.LR_PACBED, bin=BIN)
        eng.propagate_frames(0, 2)
        eng.layer_pacbed_reset()
        eng.layer_pacbed_add()
        assert eng.layer_pacbed().shape == (4, 64, 64)
        staging = eng.layer_reduce_bytes(_native.LR_BYTES_STAGING)
        eng.close()
        gc.collect()
        return torch.cuda.mem_get_info(0)[0], staging
    free = [cycle() for _ in range(3)]
    print(f"free device memory after each cycle: {[f for f, _ in free]}")
    assert abs(free[2][0] - free[0][0]) < free[0][1], free          # (the staging is the smallest buffer of the mode)
