"""Elastic / thermal-diffuse split on the MI355X: the coherent accumulation pass (msl_coherent_reset / _add / _finish) against
numpy, its refusals, run_diffraction(split=True) against the oracle, known answers, Parseval against the TACAW path, and the
frames-inside loop against the frames-outside one."""
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


# ------------------------------------------------------------------ 1. the kernels alone
KERNEL_CASES = [
    # B, T, (wx, wy), ld pad, bins, frames that nearly cancel
    (3, 5, (45, 63), 0, [(1, 1), (3, 7), (5, 9), (45, 63)], False),          # odd K: 8-byte loads
    (3, 4, (45, 63), 3, [(1, 1), (3, 7), (5, 9), (45, 63)], False),          # odd K, even ld: still 8-byte loads
    (2, 4, (32, 32), 0, [(2, 2), (4, 8), (32, 1)], False),                   # 16-byte loads
    (2, 4, (32, 32), 6, [(2, 2), (4, 8), (32, 1)], False),                   # even pad: still 16-byte loads
    (2, 4, (32, 32), 5, [(2, 2), (4, 8), (32, 1)], False),                   # odd pad: 8-byte loads
    (2, 3, (256, 256), 32, [(8, 8), (2, 64)], False),                        # more than one block of pixels
    (70, 1000, (4, 4), 0, [(1, 1), (2, 2), (4, 4), (1, 4)], False),          # B * T > 65535 rows, 1000 addends
    (2, 12, (32, 32), 0, [(1, 1), (4, 8), (32, 32)], True),                  # Psi, -Psi (1 + 1e-3), ...: the sum is 1e-3 of its addends
]


@pytest.mark.parametrize("B,T,shape,ld_pad,bins,cancel", KERNEL_CASES)
def test_coherent_sum_matches_numpy(ps, B, T, shape, ld_pad, bins, cancel):
    """|sum of the frames|^2 / n^2 per bin against the complex128 sum of the same complex64 inputs.  Bound per bin:
    1e-12 * sum_bin (sum_j |Psi_j|)^2 / n^2 -- float64 rounding over at most 1000 addends (1000 * 2.2e-16 on the sum, twice that
    on its square) with a wide margin; a single float32 step on the way (6e-8) misses it by four orders of magnitude."""
    import torch
    rng = np.random.default_rng(B * 1000 + T + ld_pad)
    wx, wy = shape
    K, ld = wx * wy, wx * wy + ld_pad
    W = (rng.standard_normal((B, T, K)) + 1j * rng.standard_normal((B, T, K))).astype(np.complex64)
    W *= rng.choice([1e-3, 1.0, 30.0], size=(B, T, 1)).astype(np.float32)
    if cancel:
        W[:, 1::2] = -W[:, 0::2] * np.float32(1.0 + 1e-3)
    host = np.full((B, T, ld), np.nan + 1j * np.nan, dtype=np.complex64)      # pad pixels must never be read
    host[:, :, :K] = W
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    W128 = W.astype(np.complex128)
    A = np.abs(W128)
    eng = _engine(wx, wy)
    try:
        src = (dW.data_ptr(), B, T, K, ld)
        first = {}
        for t0, count in [(0, 1), (0, T), (1, T - 2)]:
            S = W128[:, t0:t0 + count].sum(axis=1).reshape(B, wx, wy)
            amp = A[:, t0:t0 + count].sum(axis=1).reshape(B, wx, wy)
            eng.coherent_reset(B)
            eng.coherent_add(t0, count, src=src)
            for bx, by in bins:
                got = eng.coherent_finish(count, bin=(bx, by), shape=shape)
                want = block_sum(np.abs(S) ** 2, bx, by) / count ** 2
                bound = 1e-12 * block_sum(amp ** 2, bx, by) / count ** 2
                assert got.shape == (B, wx // bx, wy // by) and got.dtype == np.float64
                assert np.isfinite(got).all()                                  # a NaN pad pixel would show here
                ratio = (np.abs(got - want) / bound).max()
                print(f"shape {shape} ld+{ld_pad} bin {(bx, by)} frames [{t0},{t0 + count}): max |got - want| / bound {ratio:.3e}")
                assert ratio <= 1.0, (bx, by, t0, count, ratio)
                first[t0, count, bx, by] = got
        # the same sequence again: no atomics, bitwise equal (finish leaves the accumulator alone: twice in a row as well)
        eng.coherent_reset(B)
        eng.coherent_add(1, T - 2, src=src)
        for bx, by in bins:
            assert np.array_equal(eng.coherent_finish(T - 2, bin=(bx, by), shape=shape), first[1, T - 2, bx, by])
            assert np.array_equal(eng.coherent_finish(T - 2, bin=(bx, by), shape=shape), first[1, T - 2, bx, by])
        # two adds, [0, 2) and [2, T), against the bound and against one add over [0, T)
        S = W128.sum(axis=1).reshape(B, wx, wy)
        amp = A.sum(axis=1).reshape(B, wx, wy)
        eng.coherent_reset(B)
        eng.coherent_add(0, 2, src=src)
        eng.coherent_add(2, T - 2, src=src)
        for bx, by in bins:
            got = eng.coherent_finish(T, bin=(bx, by), shape=shape)
            bound = 1e-12 * block_sum(amp ** 2, bx, by) / T ** 2
            assert (np.abs(got - block_sum(np.abs(S) ** 2, bx, by) / T ** 2) <= bound).all(), (bx, by)
            assert (np.abs(got - first[0, T, bx, by]) <= bound).all(), (bx, by)
        # reset zeroes; a smaller B leaves the last probes out
        eng.coherent_reset(B)
        assert not eng.coherent_finish(1, bin=bins[0], shape=shape).any()
        eng.coherent_add(0, T, src=(dW.data_ptr(), B - 1, T, K, ld))
        got = eng.coherent_finish(T, bin=bins[0], shape=shape)
        assert np.array_equal(got[:B - 1], first[(0, T) + bins[0]][:B - 1]) and not got[B - 1].any()
        assert eng.coherent_finish(T, B=B - 1, bin=bins[0], shape=shape).shape[0] == B - 1
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. refusals
def test_coherent_refusals(ps):
    import torch
    eng = _engine(6, 8)                                                      # 48 stored pixels, accumulator rows of 64
    try:
        d = torch.zeros((2, 3, 50), dtype=torch.complex64, device="cuda")
        p = d.data_ptr()
        good = (p, 2, 3, 48, 50)
        with pytest.raises(ValueError):
            eng.coherent_add(src=good)                                       # before any reset: nothing is sized
        with pytest.raises(ValueError):
            eng.coherent_finish(1, bin=(1, 1))
        eng.coherent_reset(2)
        eng.coherent_add(src=good)
        assert eng.coherent_finish(3, bin=(3, 4)).shape == (2, 2, 2)
        for kw in (dict(src=(p, 2, 3, 48, 47)),                              # ld < K
                   dict(t0=2, count=2, src=good),                            # frame range leaves [0, T)
                   dict(t0=-1, count=1, src=good),
                   dict(t0=0, count=0, src=good),
                   dict(t0=3, count=1, src=good),
                   dict(src=(p, 3, 3, 48, 50)),                              # B beyond the last reset
                   dict(src=(p, 2, 3, 65, 70)),                              # K beyond the accumulator's rows
                   dict(src=(p, 2, 3, 40, 50)),                              # K differs from the adds since the reset
                   dict(src=(p, 0, 3, 48, 50))):
            with pytest.raises(ValueError):
                eng.coherent_add(**kw)
        for kw in (dict(n=3, bin=(4, 1)),                                    # bx does not divide wx
                   dict(n=3, bin=(1, 3)),                                    # by does not divide wy
                   dict(n=3, bin=(0, 1)),
                   dict(n=0, bin=(1, 1)),                                    # n >= 1
                   dict(n=3, B=3, bin=(1, 1)),                               # B beyond the last reset
                   dict(n=3, bin=(1, 1), shape=(5, 8)),                      # not the rows that were added
                   dict(n=3, bin=(1, 1), shape=(9, 8))):                     # more pixels than the accumulator's rows
            with pytest.raises(ValueError):
                eng.coherent_finish(**kw)
        with pytest.raises(RuntimeError):
            eng.coherent_add()                                               # no wavefunction ring: MSL_ERR_STATE
        eng.coherent_reset()                                                 # B <= 0: n_probes
        assert eng.coherent_finish(1).shape == (1, 6, 8)
        with pytest.raises(ValueError):
            eng.coherent_add(src=good)                                       # two probes into an accumulator of one
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. the oracle
def _oracle_case(ps, **traj_kw):
    from oracle import multislice_oracle as orc
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, traj_kw.pop("nz", 6), traj_kw.pop("n_frames", 3), ny=80, seed=11, **traj_kw)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    rng = np.random.default_rng(12)
    pp = [tuple(v) for v in rng.random((20, 2)) * [lx, ly]]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp, workers=orc.usable_cores())
    return tr, pp, want["wavefunction_data"][..., 0]


@pytest.fixture(scope="module")
def oracle_cases(ps):
    """"weak": the case of test_gpu_diffraction.py (21 light atoms in 3 A, 0.03 A displacements), whose diffuse part is below
    1e-3 of the total.  "strong": 60 slices of gold-like atoms at twice the density with 0.3 A displacements, chosen with the
    oracle so that ||tds|| >= 0.1 ||total|| for every probe, window and bin below (the smallest ratio is 0.247)."""
    return {"weak": _oracle_case(ps, density=0.1),
            "strong": _oracle_case(ps, nz=60, density=0.2, amplitude=0.3, species=(79,))}


def _split_run(ps, tr, pp, bin, **kw):
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=bin, split=True), **kw)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    return calc, calc.run_diffraction()


@pytest.mark.parametrize("which", ["weak", "strong"])
@pytest.mark.parametrize("k_window,frame_batch,probe_batch,bin", [(None, 1, 8, (1, 1)), (None, 3, 20, (4, 5)),
                                                                  ((48, 40), 2, 7, (6, 8)), ((33, 27), 2, 7, (3, 9))])
def test_split_matches_oracle(ps, oracle_cases, which, k_window, frame_batch, probe_batch, bin):
    tr, pp, wf = oracle_cases[which]
    calc, dd = _split_run(ps, tr, pp, bin, probe_batch=probe_batch, k_window=k_window, frame_batch=frame_batch)
    assert calc._engine.frame_batch == frame_batch and calc.probe_batch == probe_batch
    nx, ny = wf.shape[-2:]
    if k_window is not None:
        x0, y0 = nx // 2 - k_window[0] // 2, ny // 2 - k_window[1] // 2
        wf = wf[..., x0:x0 + k_window[0], y0:y0 + k_window[1]]
    wf = wf.astype(np.complex128)
    total = block_sum((np.abs(wf) ** 2).mean(axis=1), *bin)
    elastic = block_sum(np.abs(wf.mean(axis=1)) ** 2, *bin)
    tds = total - elastic
    assert dd.elastic.shape == total.shape and dd.elastic.dtype == np.float64
    assert dd.intensity.shape == total.shape and dd.n_frames == 3 and dd.stem is None
    norm = lambda a: np.linalg.norm(a.ravel())
    share = min(norm(tds[p]) / norm(total[p]) for p in range(20))
    if which == "strong":
        assert share >= 0.1, share
    e_tot = max(rel_l2(dd.intensity[p], total[p]) for p in range(20))
    e_el = max(rel_l2(dd.elastic[p], elastic[p]) for p in range(20))
    e_tds = max(norm(dd.tds[p] - tds[p]) / norm(total[p]) for p in range(20))
    low = (dd.tds / np.where(dd.intensity > 0, dd.intensity, 1.0)).min()
    print(f"{which} window {k_window} batches ({frame_batch},{probe_batch}) bin {bin}: min ||tds|| / ||total|| {share:.3e}; max per pattern: "
          f"total rel-L2 {e_tot:.3e}, elastic rel-L2 {e_el:.3e}, ||tds err|| / ||total|| {e_tds:.3e}; min tds / intensity {low:.3e}")
    assert e_tot <= 2e-4
    assert e_el <= 2e-4
    assert e_tds <= 4e-4
    assert (dd.tds >= -2e-6 * dd.intensity).all()
    assert np.array_equal(dd.part("elastic").pacbed(), dd.elastic.mean(axis=0))


# ------------------------------------------------------------------ 4. known answers
@pytest.mark.parametrize("n_frames,amplitude,frame_batch,probe_batch,bin", [(1, 0.03, 1, 7, (1, 1)), (1, 0.03, 1, 20, (4, 5)),
                                                                            (3, 0.0, 2, 8, (1, 1)), (3, 0.0, 1, 7, (4, 5))])
def test_nothing_is_diffuse_without_motion(ps, n_frames, amplitude, frame_batch, probe_batch, bin):
    """one frame, or three equal ones: <|Psi|^2> = |<Psi>|^2, so tds is the rounding of the two passes -- twice the 1e-6 per-bin
    contract of the diffraction pass"""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, n_frames, ny=80, density=0.1, seed=11, amplitude=amplitude)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(12).random((20, 2)) * [lx, ly]]
    calc, dd = _split_run(ps, tr, pp, bin, probe_batch=probe_batch, frame_batch=frame_batch)
    assert dd.elastic.shape == (20, 96 // bin[0], 80 // bin[1]) and (dd.intensity > 0).any()
    worst = (np.abs(dd.tds) / np.where(dd.intensity > 0, dd.intensity, 1.0)).max()
    print(f"T {n_frames} amplitude {amplitude} batches ({frame_batch},{probe_batch}) bin {bin}: max |tds| / intensity {worst:.3e}")
    assert (np.abs(dd.tds) <= 2e-6 * dd.intensity).all()


# ------------------------------------------------------------------ 5. Parseval against the TACAW path
def test_tds_is_the_energy_integrated_tacaw_intensity(ps, oracle_cases):
    """sum over frequency of |FFT_t (Psi - <Psi>)|^2 = T sum_t |Psi|^2 - |sum_t Psi|^2 = T^2 tds: the normalisation of the split
    against run() + TACAWData, which the goldens pin"""
    for which in ("weak", "strong"):
        tr, pp, _ = oracle_cases[which]
        T = tr.n_frames
        calc = ps.MultisliceCalculator(progress=False)
        calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        tac = ps.TACAWData(calc.run())
        want = npy(tac.intensity).astype(np.float64).sum(axis=1) / T ** 2
        _, dd = _split_run(ps, tr, pp, (1, 1), probe_batch=7, frame_batch=2)
        assert want.shape == dd.tds.shape
        norm = lambda a: np.linalg.norm(a.ravel())
        err = max(norm(dd.tds[p] - want[p]) / norm(dd.intensity[p]) for p in range(20))
        print(f"{which}: max ||tds - sum_w I / T^2|| / ||total|| per pattern {err:.3e}; "
              f"max ||tds|| / ||total|| {max(norm(dd.tds[p]) / norm(dd.intensity[p]) for p in range(20)):.3e}")
        assert err <= 4e-4


# ------------------------------------------------------------------ 6. the new loop leaves the old results alone
def test_split_run_reproduces_the_plain_run(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    D = ps.Detector
    tr = synthetic_trajectory(64, 5, 3, density=0.1, seed=21)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = [tuple(v) for v in np.random.default_rng(22).random((19, 2)) * [lx, ly]]
    dets = [D("bf", outer=25.0), D("adf", inner=40.0, outer=150.0), D("haadf", inner=40.0, signal="amplitude"), D("comx", signal="com_x")]
    out = {}
    for split in (False, True):
        calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=(2, 4), split=split), detectors=dets, probe_batch=7,
                                       frame_batch=2)
        calc.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
        out[split] = calc.run_diffraction()
    plain, both = out[False], out[True]
    assert plain.elastic is None and both.elastic is not None
    scale = plain.intensity.max(axis=(-2, -1), keepdims=True)
    err = (np.abs(both.intensity - plain.intensity) / scale).max()
    assert both.stem is not None and both.stem.signals.shape == plain.stem.signals.shape == (19, 3, 4)
    serr = (np.abs(both.stem.signals - plain.stem.signals).max(axis=(0, 1)) / np.abs(plain.stem.signals).max(axis=(0, 1))).max()
    print(f"split against plain: intensity max diff / pattern max {err:.3e}, detector signals max diff / signal max {serr:.3e}")
    assert err <= 1e-6
    assert serr <= 1e-6


def test_batches_give_the_same_elastic_patterns(ps, oracle_cases):
    tr, pp, _ = oracle_cases["strong"]
    out = {}
    for pb in (7, 20):
        for fb in (1, 3):
            out[pb, fb] = _split_run(ps, tr, pp, (4, 5), probe_batch=pb, frame_batch=fb)[1].elastic
    ref = out[20, 3]
    scale = ref.max(axis=(-2, -1), keepdims=True)
    for key, o in out.items():
        err = (np.abs(o - ref) / scale).max()
        print(f"probe_batch, frame_batch {key}: elastic max diff / pattern max {err:.3e}")
        assert err <= 1e-6, key
