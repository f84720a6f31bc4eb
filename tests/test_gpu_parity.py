"""GPU parity tests: the HIP path (through the C ABI) against the reference goldens and the oracle.

Run on the MI355X box with `pytest -m gpu`.  Tolerances are the stated fp32 contract of
SURVEY.md section 8c:
    exit wave / wavefunction  rel-L2 <= 1e-4  and reference residual sum((|F|-|D|)^2)/sum(|F|^2) <= 1e-6
    potential                 max|dV| / max|V| <= 1e-5
    TACAW intensity           rel-L2 <= 2e-4
"""
import os

import numpy as np
import pytest

from conftest import rel_l2, ref_residual

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4
RESID_TOL = 1e-6
POT_TOL = 1e-5
TACAW_TOL = 2e-4


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


def _prime_factors(n):
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p); n //= p
        p += 1
    if n > 1:
        out.append(n)
    return out or [1]


# ------------------------------------------------------------------ FFT kernels alone
@pytest.mark.parametrize("shape,batch", [((64, 64), 3), ((96, 80), 2), ((45, 63), 2), ((256, 256), 2), ((128, 512), 1),
                                         ((1024, 1024), 2), ((2048, 2048), 1), ((330, 200), 1), ((2, 2), 1),
                                         ((1024, 256), 3), ((256, 1024), 3), ((1024, 64), 2), ((40, 256), 2),
                                         ((501, 491), 2), ((167, 64), 2), ((1024, 997), 1), ((4093, 34), 1)])
def test_fft2_matches_numpy(ps, shape, batch):
    from pyslice_amd import _native
    rng = np.random.default_rng(5)
    a = (rng.standard_normal((batch,) + shape) + 1j * rng.standard_normal((batch,) + shape)).astype(np.complex64)
    eng = _native.Engine(shape[0], shape[1], 1, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=1)
    f = eng.fft2(a, +1)
    want = np.fft.fft2(a.astype(np.complex128), axes=(1, 2))
    tol = 3e-6 if all(max(_prime_factors(n)) <= 13 for n in shape) else 1e-5      # Bluestein lines: two FFTs of >= 2N
    assert rel_l2(f, want) < tol
    b = eng.fft2(f, -1)
    assert rel_l2(b, a) < tol
    eng.close()


@pytest.mark.parametrize("n,nz,P", [(256, 12, 5), (1024, 6, 3)])
def test_fourstep_kernels_match_generic_kernels(ps, n, nz, P):
    """The register-resident four-step passes (fft_path=0) against the generic LDS Stockham passes (fft_path=1)
    on the same frame: potential, slice loop and fused exit-wave epilogue."""
    from pyslice_amd import _native
    from pyslice_amd.synthetic import synthetic_trajectory
    from pyslice_amd.potentials import slice_edges
    tr = synthetic_trajectory(n, nz, 1, seed=11)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = np.random.default_rng(1).random((P, 2)) * [lx, ly]
    outs = []
    for path in (0, 1):
        eng = _native.Engine(n, n, nz, xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], 0.0370144, 9.24396e-4,
                             n_probes=P, n_frames=1, fft_path=path)
        eng.set_kirkland(ps.loadKirkland())
        eng.set_slices(*slice_edges(zs))
        eng.set_probes(30.0, pp)
        eng.build_potential(tr.positions[0], tr.atom_types.astype(np.int32))
        eng.propagate()
        ex = eng.exit_waves()
        eng.propagate_frame(0)
        outs.append((eng.probes(), ex, eng.wavefunction()))
        eng.close()
    for a, b in zip(outs[0], outs[1]):
        assert rel_l2(a, b) < 5e-6


def test_unsupported_length_fails_loudly(ps):
    from pyslice_amd import _native
    with pytest.raises(NotImplementedError):
        _native.Engine(4099, 64, 1, 0.1, 0.1, 0.5, 0.037, 1e-3)      # prime > 4096: beyond the LDS-resident Bluestein path


# ------------------------------------------------------------------ goldens
def test_g3_form_factor(ps, golden):
    from pyslice_amd import _native
    g = golden("g3_formfactor")
    Zs = g["Z"]
    eng = _native.Engine(32, 32, 1, 0.1, 0.1, 0.5, 0.037, 1e-3, keep_potential=True)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(np.array([0.0]), np.array([0.5]))
    pos = np.tile(np.array([[0.5, 0.5, 0.1]]), (len(Zs), 1))
    eng.build_potential(pos, Zs.astype(np.int32))
    ff = eng.form_factors(len(Zs))          # species sorted ascending == golden order
    for i in range(len(Zs)):
        assert rel_l2(ff[i], g["f"][i]) < 2e-7
    eng.close()


@pytest.mark.parametrize("name", ["g4_potential_64", "g4_potential_96x80", "g4_potential_axis0"])
def test_g4_potential(ps, golden, orc, name):
    g = golden(name)
    xs, ys, zs, *_ = orc.grid_from_box(g["box"], 0.1, 0.5)
    pot = ps.Potential(xs, ys, zs, g["positions"], list(g["Z"]), kind="kirkland", slice_axis=int(g["slice_axis"]))
    V = npy(pot.array)
    assert V.shape == g["V"].shape and V.dtype == np.float64
    assert np.abs(V - g["V"]).max() / np.abs(g["V"]).max() < POT_TOL
    # element-name input takes the same path
    names = ["B" if z == 5 else "N" for z in g["Z"]]
    V2 = npy(ps.Potential(xs, ys, zs, g["positions"], names, slice_axis=int(g["slice_axis"])).array)
    assert np.array_equal(V, V2)


def test_g5_probes(ps, golden):
    g = golden("g5_probes")
    xs, ys, pp, eV = g["xs"], g["ys"], g["positions"], float(g["eV"])
    for mrad in (0, 5, 30):
        pr = ps.Probe(xs, ys, mrad, eV)
        base = npy(pr.array)
        assert base.shape == g[f"base_{mrad}"].shape
        assert rel_l2(base, g[f"base_{mrad}"]) < 2e-6
        bp = ps.create_batched_probes(pr, pp)
        assert rel_l2(npy(bp.array), g[f"batch_{mrad}"]) < 2e-6
    assert npy(ps.Probe(xs, ys, 0, eV).array).dtype == np.float64      # Q5
    g2 = golden("g5_probes_96x80")
    bp = ps.create_batched_probes(ps.Probe(g2["xs"], g2["ys"], 30, eV), g2["positions"])
    assert rel_l2(npy(bp.array), g2["batch_30"]) < 2e-6
    # a probe built from a caller array is shifted through fft2 * ramp * ifft2 on the device
    custom = ps.Probe(xs, ys, 30, eV, array=g["base_30"])
    bc = ps.create_batched_probes(custom, pp)
    assert rel_l2(npy(bc.array), g["batch_30"]) < 3e-6


@pytest.mark.parametrize("name", ["g6_propagate_64_single", "g6_propagate_64_batch", "g6_propagate_64_plane",
                                  "g6_propagate_96x80_batch"])
def test_g6_propagate(ps, golden, name):
    g = golden(name)
    xs, ys, zs, eV = g["xs"], g["ys"], g["zs"], float(g["eV"])
    # the golden carries V itself: upload it so that this test isolates the slice loop
    pot = ps.Potential(xs, ys, zs, np.zeros((0, 3)), [], kind="kirkland")
    pot.array = g["V"]
    pr = ps.create_batched_probes(ps.Probe(xs, ys, float(g["mrad"]), eV), g["positions"])
    ex = npy(ps.Propagate(pr, pot))
    want = g["exit"]
    if want.shape[0] == 1:
        assert ex.ndim == 2                      # Q13: single probe comes back squeezed
        ex = ex[None]
    assert ex.dtype == np.complex128
    assert rel_l2(ex, want) < WAVE_TOL
    assert ref_residual(ex, want) < RESID_TOL


@pytest.mark.parametrize("name", ["g7_calculator_64", "g7_calculator_32_default_probe"])
def test_g7_calculator(ps, golden, name):
    g = golden(name)
    pos = g["positions"]
    tr = ps.Trajectory(g["Z"], pos, np.zeros_like(pos), g["box"], 0.005)
    calc = ps.MultisliceCalculator(progress=False)
    pp = [tuple(p) for p in g["probe_positions"]] if name == "g7_calculator_64" else None
    calc.setup(tr, aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), sampling=0.1, slice_thickness=0.5,
               probe_positions=pp)
    wf = calc.run()
    data = npy(wf.wavefunction_data)
    assert data.shape == g["wavefunction_data"].shape and data.dtype == np.complex128
    assert rel_l2(data, g["wavefunction_data"]) < WAVE_TOL
    assert ref_residual(data, g["wavefunction_data"]) < RESID_TOL
    assert np.array_equal(npy(wf.kxs), g["kxs"]) and npy(wf.kxs).dtype == np.float32      # Q2
    assert np.array_equal(npy(wf.kys), g["kys"])
    assert np.allclose(wf.time, g["time"], rtol=0, atol=0)
    assert np.allclose(np.asarray(wf.probe_positions, dtype=float), g["probe_positions"])
    assert list(wf.layer) == [0]


def test_g8_tacaw(ps, golden):
    g = golden("g8_tacaw_32")
    pos = g["positions"]
    tr = ps.Trajectory(g["Z"], pos, np.zeros_like(pos), g["box"], 0.005)
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), probe_positions=[tuple(p) for p in g["probe_positions"]])
    wf = calc.run()
    tac = ps.TACAWData(wf)
    assert np.allclose(tac.frequencies, g["frequencies"], rtol=1e-15)
    inten = npy(tac.intensity)
    assert inten.shape == g["intensity"].shape
    assert rel_l2(inten, g["intensity"]) < TACAW_TOL
    assert rel_l2(tac.spectrum(0), g["spectrum0"]) < TACAW_TOL
    assert rel_l2(tac.spectrum(None), g["spectrum_all"]) < TACAW_TOL
    assert rel_l2(tac.diffraction(0), g["diffraction0"]) < TACAW_TOL
    assert rel_l2(tac.diffraction(None), g["diffraction_all"]) < TACAW_TOL
    assert rel_l2(tac.spectrum_image(25.0), g["spectrum_image_25"]) < TACAW_TOL
    assert rel_l2(tac.spectral_diffraction(25.0, 1), g["spectral_diffraction_25"]) < TACAW_TOL
    T = len(g["time"])
    assert inten[:, T // 2].max() == 0.0                    # K5: DC bin of the mean-subtracted series
    with pytest.raises(ValueError):
        ps.TACAWData(wf, layer_index=2)
    # the multi-process path (all-to-all of frame shards, msl_tacaw on torch memory) degenerates to identity
    # exchanges at world size 1: exercises the zero-copy views and the external-pointer entry
    wf3 = ps.WFData(probe_positions=wf.probe_positions, time=wf.time, kxs=wf.kxs, kys=wf.kys, layer=wf.layer,
                    wavefunction_data=None, probe=wf.probe)
    wf3._engine, wf3._resident, wf3._output, wf3._frame_shard = calc._engine, False, "host", (T, T)
    tac3 = ps.TACAWData(wf3)
    assert rel_l2(npy(tac3.intensity), g["intensity"]) < TACAW_TOL
    # the staged path (WFData not resident on the device) gives the same numbers
    wf2 = ps.WFData(probe_positions=wf.probe_positions, time=wf.time, kxs=wf.kxs, kys=wf.kys, layer=wf.layer,
                    wavefunction_data=g["wavefunction_data"], probe=wf.probe)
    tac2 = ps.TACAWData(wf2)
    assert rel_l2(npy(tac2.intensity), g["intensity"]) < TACAW_TOL
    # reductions (device kernels) from all three intensity sources; expectations restated on the golden intensity
    I = g["intensity"]
    kxs, kys = npy(wf.kxs), npy(wf.kys)
    mask = (np.sqrt(kxs[:, None] ** 2 + kys[None, :] ** 2) < 2.0)
    fi = int(np.argmin(np.abs(g["frequencies"] - 25.0)))
    kxp, kyp = np.linspace(-3, 3, 7), np.linspace(0, 2.5, 7)
    ix = [int(np.argmin(np.abs(kxs - v))) for v in kxp]
    iy = [int(np.argmin(np.abs(kys - v))) for v in kyp]
    for t in (tac, tac2, tac3):
        assert rel_l2(t.spectrum(1), g["intensity"][1].sum(axis=(1, 2))) < TACAW_TOL
        assert rel_l2(t.diffraction(None), g["diffraction_all"]) < TACAW_TOL
        assert rel_l2(t.spectral_diffraction(25.0), I[:, fi].mean(axis=0)) < TACAW_TOL
        assert rel_l2(t.masked_spectrum(mask, 0), (I[0] * mask[None]).sum(axis=(1, 2))) < TACAW_TOL
        assert rel_l2(t.masked_spectrum(mask), (I * mask[None, None]).sum(axis=(2, 3)).mean(axis=0)) < TACAW_TOL
        assert rel_l2(t.masked_spectrum(mask * 0.5, 1), 0.5 * (I[1] * mask[None]).sum(axis=(1, 2))) < TACAW_TOL
        soft = np.exp(-(kxs[:, None] ** 2 + kys[None, :] ** 2) / 2.0)          # a smooth detector function: every weight distinct
        assert rel_l2(t.masked_spectrum(soft, 1), (I[1] * soft[None]).sum(axis=(1, 2))) < TACAW_TOL
        assert rel_l2(t.masked_spectrum(soft), (I * soft[None, None]).sum(axis=(2, 3)).mean(axis=0)) < TACAW_TOL
        assert rel_l2(t.dispersion(kxp, kyp, 1), I[1][:, ix, iy]) < TACAW_TOL
        assert rel_l2(t.dispersion(kxp, kyp), I[:, :, ix, iy].mean(axis=0)) < TACAW_TOL
        assert t.dispersion(kxp, kyp[:3]).shape == (len(g["frequencies"]), 7)
        with pytest.raises(ValueError):
            t.spectrum(99)
        with pytest.raises(ValueError):
            t.masked_spectrum(mask[:-1])


def test_g9_haadf(ps, golden):
    g = golden("g9_haadf_32")
    pos = g["positions"]
    tr = ps.Trajectory(g["Z"], pos, np.zeros_like(pos), g["box"], 0.005)
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), probe_positions=g["probe_positions"])
    wf = calc.run()
    wf.probe_positions = np.asarray(wf.probe_positions)
    adf = ps.HAADFData(wf).calculateADF(collection_angle=float(g["collection_angle"]))
    assert adf.shape == g["adf"].shape
    assert rel_l2(adf, g["adf"]) < 1e-4
    # staged path: a WFData that is not resident on the device (e.g. gathered shards, arrays from disk)
    wf2 = ps.WFData(probe_positions=wf.probe_positions, time=wf.time, kxs=wf.kxs, kys=wf.kys, layer=wf.layer,
                    wavefunction_data=npy(wf.wavefunction_data), probe=wf.probe)
    adf2 = ps.HAADFData(wf2).calculateADF(collection_angle=float(g["collection_angle"]))
    assert rel_l2(adf2, g["adf"]) < 1e-4


@pytest.mark.parametrize("B,F,shape", [(3, 5, (45, 63)), (2, 16, (256, 256)), (1, 3, (6, 7)), (70, 1000, (4, 4))])
def test_reduction_kernels_match_numpy(ps, B, F, shape):
    """msl_tacaw_spectrum / _diffraction / _dispersion / msl_adf on caller-held device memory: odd K (scalar loads),
    K % 4 == 0 (16-byte loads), chunked rows, more than 65535 rows."""
    import torch
    from pyslice_amd import _native
    rng = np.random.default_rng(B * 100 + F)
    K = shape[0] * shape[1]
    I = rng.random((B, F, K), dtype=np.float32) * rng.choice([1e-3, 1.0, 50.0], size=(B, F, 1)).astype(np.float32)
    W = (rng.standard_normal((B, F, K)) + 1j * rng.standard_normal((B, F, K))).astype(np.complex64)
    mask = rng.random(K) < 0.4
    dI, dW = torch.from_numpy(I).cuda(), torch.from_numpy(W).cuda()
    torch.cuda.synchronize()
    eng = _native.Engine(2, 2, 1, 1.0, 1.0, 1.0, 1.0, 0.0, n_probes=1, n_frames=0, device=0)
    src = (dI.data_ptr(), B, F, K)
    I64 = I.astype(np.float64)
    assert rel_l2(eng.tacaw_spectrum(src=src), I64.sum(axis=2)) < 1e-6
    assert rel_l2(eng.tacaw_spectrum(mask, src=src), (I64 * mask).sum(axis=2)) < 1e-6
    assert rel_l2(eng.tacaw_diffraction(src=src), I64.sum(axis=(0, 1))) < 1e-6
    b1, f0 = max(1, B // 2), F // 3
    assert rel_l2(eng.tacaw_diffraction(probes=(0, b1), freqs=(f0, F), scale=0.25, src=src), 0.25 * I64[:b1, f0:].sum(axis=(0, 1))) < 1e-6
    idx = rng.integers(0, K, size=11)
    assert np.array_equal(eng.tacaw_dispersion(idx, src=src), I[:, :, idx])
    assert rel_l2(eng.adf(mask, src=(dW.data_ptr(), B, F, K)), (np.abs(W.astype(np.complex128)) * mask).sum(axis=2).mean(axis=1)) < 1e-6
    with pytest.raises(ValueError):
        eng.tacaw_dispersion([K], src=src)
    with pytest.raises(ValueError):
        eng.tacaw_diffraction(probes=(0, B + 1), src=src)
    with pytest.raises(RuntimeError):
        eng.tacaw_spectrum()                     # no resident intensity on this handle
    eng.close()


# ------------------------------------------------------------------ oracle on seeded inputs, larger grids
def _oracle_case(ps, orc, n, nz, P, mrad, density, seed):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(n, nz, 1, density=density, seed=seed)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    assert (len(xs), len(ys), len(zs)) == (n, n, nz)
    rng = np.random.default_rng(seed + 7)
    pp = [(lx / 2, ly / 2)] if P == 1 else [tuple(v) for v in rng.random((P, 2)) * [lx, ly]]
    V = orc.potential(xs, ys, zs, tr.positions[0], tr.atom_types)
    pr = orc.batched_probes(orc.probe_array(xs, ys, mrad, 100e3), xs, ys, pp)
    ex = orc.propagate(pr, V, xs, ys, zs, 100e3)
    pot = ps.Potential(xs, ys, zs, tr.positions[0], list(tr.atom_types))
    Vg = npy(pot.array)
    gex = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(xs, ys, mrad, 100e3), pp), pot))
    if gex.ndim == 2:
        gex = gex[None]
    return V, Vg, ex, gex


@pytest.mark.parametrize("n,nz,P,mrad", [(128, 12, 3, 30.0), (256, 50, 1, 30.0), (256, 50, 2, 0.0)])
def test_oracle_parity_midsize(ps, orc, n, nz, P, mrad):
    V, Vg, ex, gex = _oracle_case(ps, orc, n, nz, P, mrad, density=0.102, seed=3)
    assert np.abs(V - Vg).max() / np.abs(V).max() < POT_TOL
    assert rel_l2(gex, ex) < WAVE_TOL
    assert ref_residual(gex, ex) < RESID_TOL


@pytest.mark.parametrize("n,nz,P", [(256, 7, 3), (256, 8, 2), (256, 1, 2), (256, 2, 1)])
def test_calculator_oracle_parity_onepass(ps, orc, n, nz, P):
    """MultisliceCalculator on a four-step grid takes the one-pass-per-slice loop (alternating transposing passes);
    odd and even slice counts start along different axes, nz = 1 and 2 are the degenerate cases."""
    from pyslice_amd.synthetic import synthetic_trajectory
    from pyslice_amd import _native
    tr = synthetic_trajectory(n, nz, 2, density=0.05, seed=21 + nz)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(3).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    got = npy(wf.wavefunction_data)
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL
    # the transmission functions come back in natural orientation whatever the internal layout
    t = calc._engine.download(_native.BUF_TRANSMISSION, np.complex64, (calc.nz, n, n))
    xs, ys, zs, *_ = orc.grid_from_box(tr.box_matrix)
    V = orc.potential(xs, ys, zs, tr.positions[-1], tr.atom_types)
    assert rel_l2(t, np.exp(1j * orc.interaction_sigma(100e3) * np.moveaxis(V, 2, 0))) < 1e-4


@pytest.mark.parametrize("nx,ny,nz,P,B", [(256, 256, 5, 1, 4), (256, 256, 4, 3, 2), (512, 512, 3, 1, 3), (512, 512, 4, 2, 4),
                                          (1024, 1024, 3, 1, 2), (1024, 256, 4, 1, 3), (96, 80, 3, 2, 4), (45, 63, 2, 1, 5),
                                          (501, 64, 2, 1, 2), (2048, 512, 2, 1, 2), (256, 256, 1, 1, 4), (700, 300, 3, 2, 3)])
def test_frame_batching_matches_oracle(ps, orc, nx, ny, nz, P, B):
    """frame_batch = B: B MD frames share every slice-loop launch (image = frame x probe, one transmission stack per
    frame).  5 frames, so the last batch is short; register kernels (256, 512, 1024, 2048 lines), the generic kernel and
    Bluestein lines; against the oracle, and bit-identical to the unbatched run."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 5, ny=ny, density=0.05, seed=90 + nz)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(4).random((P, 2)) * [lx, ly]]
    out = []
    for fb in (B, 1):
        calc = ps.MultisliceCalculator(progress=False, dtype="complex64", frame_batch=fb)
        calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        assert calc._engine.frame_batch == fb
        out.append(npy(calc.run().wavefunction_data))
    assert np.array_equal(out[0], out[1])
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(out[0], want) < WAVE_TOL


def test_frame_batching_default_for_single_probe_runs(ps, orc):
    """the reference's default (probe_positions=None: one probe) batches frames automatically; results unchanged"""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(256, 6, 70, density=0.03, seed=12)
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3)
    from pyslice_amd.calculators import default_frame_batch
    assert default_frame_batch(1, 6, 256, 256) == 256 and default_frame_batch(64, 200, 1024, 1024) == 4
    assert calc._engine.frame_batch == 70            # about 256 images per launch, capped by the run's 70 frames
    got = npy(calc.run().wavefunction_data)
    idx = [0, 1, 63, 64, 69]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, None, frames=idx)["wavefunction_data"]
    assert rel_l2(got[:, idx], want) < WAVE_TOL


def test_calculator_oracle_parity_onepass_nonsquare(ps, orc):
    """256 x 1024 grid: the transposing passes alternate between the R=16 (x lines) and R=32 (y lines) kernels."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(256, 6, 1, ny=1024, density=0.03, seed=31)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    assert (len(xs), len(ys), len(zs)) == (256, 1024, 6)
    pp = [(lx / 2, ly / 2), (3.3, 70.1), (20.0, 5.0)]
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert calc._engine is not None
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(512, 512, 5, 3), (512, 512, 4, 2), (512, 512, 1, 2), (1024, 512, 3, 2),
                                         (512, 256, 6, 2), (2048, 256, 4, 2), (256, 2048, 3, 2), (2048, 2048, 3, 1)])
def test_calculator_oracle_parity_onepass_2r2_lengths(ps, orc, nx, ny, nz, P):
    """Grid lengths 512 = 2*16^2 and 2048 = 2*32^2: one transposing pass per slice with a radix-2 step around the
    four-step transform; passes start along y, an odd slice count ends with one plain transpose."""
    from pyslice_amd.synthetic import synthetic_trajectory
    from pyslice_amd import _native
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.02 if nx * ny < 2 ** 21 else 0.004, seed=41 + nz)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    assert (len(xs), len(ys), len(zs)) == (nx, ny, nz)
    pp = [(lx / 2, ly / 2), (3.3, 0.4 * ly), (0.7 * lx, 5.0)][:P]
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL
    t = calc._engine.download(_native.BUF_TRANSMISSION, np.complex64, (nz, nx, ny))
    V = orc.potential(xs, ys, zs, tr.positions[-1], tr.atom_types)
    assert rel_l2(t, np.exp(1j * orc.interaction_sigma(100e3) * np.moveaxis(V, 2, 0))) < 1e-4


@pytest.mark.parametrize("nx,ny,nz,window", [(256, 256, 4, (64, 96)), (256, 256, 3, (50, 40)), (128, 96, 3, (33, 64)),
                                              (512, 512, 3, (128, 64)), (256, 1024, 2, (256, 128)), (64, 64, 2, (64, 1))])
def test_k_window_is_a_crop_of_the_full_spectrum(ps, orc, nx, ny, nz, window):
    """k_window=(wx,wy) keeps the central pixels of fftshift(fft2(exit)): equal to cropping the oracle's full result;
    aligned windows on four-step grids only transform the kept columns, other shapes go through the generic store.
    TACAW is per pixel, so TACAWData on the window equals the crop of the full intensity."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 4, ny=ny, density=0.03, seed=77)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [(lx / 2, ly / 2), (0.3 * lx, 0.8 * ly)]
    calc = ps.MultisliceCalculator(progress=False, k_window=window)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    wx, wy = window
    x0, y0 = nx // 2 - wx // 2, ny // 2 - wy // 2
    ref = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)
    full_wf = ref["wavefunction_data"]
    want = full_wf[:, :, x0:x0 + wx, y0:y0 + wy]
    got = npy(wf.wavefunction_data)
    assert got.shape == (2, 4, wx, wy, 1)
    scale = np.linalg.norm(full_wf) * np.sqrt(wx * wy / (nx * ny))
    assert np.linalg.norm(got - want) / max(np.linalg.norm(want), scale) < WAVE_TOL
    kxs, kys, time = orc.wf_axes(nx, ny, 0.1, 4, tr.timestep)
    assert np.allclose(npy(wf.kxs), kxs[x0:x0 + wx]) and np.allclose(npy(wf.kys), kys[y0:y0 + wy])
    tac = ps.TACAWData(wf)
    _, full_I = orc.tacaw(full_wf, time)
    want_I = full_I[:, :, x0:x0 + wx, y0:y0 + wy]
    got_I = npy(tac.intensity)
    assert got_I.shape == want_I.shape
    assert np.linalg.norm(got_I - want_I) / max(np.linalg.norm(want_I), 1e-30) < TACAW_TOL
    assert rel_l2(tac.spectrum(1), want_I[1].sum(axis=(1, 2))) < TACAW_TOL
    assert rel_l2(tac.diffraction(None), want_I.sum(axis=1).mean(axis=0)) < TACAW_TOL


@pytest.mark.parametrize("nx,ny,nz", [(512, 256, 5), (256, 512, 4), (96, 80, 3), (1024, 256, 2), (2048, 2048, 6),
                                       (2048, 512, 9), (500, 2048, 4)])
def test_engine_uploaded_potential_changed_beam_onepass(ps, orc, nx, ny, nz):
    """C-ABI level: msl_set_beam after creation (propagator tables, also the split-order ones of 512-point lines),
    msl_upload_potential (every x-pass slice transposed on upload) and msl_propagate leaving real-space exit waves,
    on grids that mix the register kernels, the 2R^2 kernels and the generic kernel."""
    from pyslice_amd import _native
    rng = np.random.default_rng(nx + nz)
    dx, dy, dz = 0.1, 0.1, 0.5
    xs, ys, zs = np.arange(nx) * dx, np.arange(ny) * dy, np.arange(nz) * dz
    V = (rng.random((nx, ny, nz)) ** 8 * 4000.0)                      # sparse peaks, a few kV.A like atoms
    eng = _native.Engine(nx, ny, nz, dx, dy, dz, orc.wavelength(60e3), orc.interaction_sigma(60e3), n_probes=3, n_frames=0)
    eng.set_beam(orc.wavelength(200e3), orc.interaction_sigma(200e3), dz)
    eng.upload_potential(np.moveaxis(V, 2, 0).astype(np.float32))
    pp = [(xs[-1] / 2, ys[-1] / 2), (3.0, 2.0), (0.0, 7.7)]
    eng.set_probes(25.0, pp)
    eng.propagate()
    got = eng.exit_waves()
    probes = orc.batched_probes(orc.probe_array(xs, ys, 25.0, 200e3), xs, ys, pp)
    want = orc.propagate(probes, V.astype(np.float32).astype(np.float64), xs, ys, zs, 200e3)
    assert rel_l2(got, want) < WAVE_TOL
    t = eng.transmission()
    assert rel_l2(t, np.exp(1j * orc.interaction_sigma(200e3) * np.moveaxis(V.astype(np.float32), 2, 0))) < 1e-5
    eng.close()


def _deep():
    import importlib.util
    spec = importlib.util.spec_from_file_location("deep", os.path.join(os.path.dirname(__file__), "..", "tools", "deep_stack_parity.py"))
    deep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(deep)
    return deep


@pytest.mark.parametrize("n,nz", [(256, 400), (512, 400), (1024, 400), (2048, 40), (501, 400), (700, 200), (100, 400)])      # (2048^2 x 400: test_config_c5_grid_2048_400_slices)
def test_deep_stack_error_growth_stays_inside_the_contract(ps, orc, n, nz):
    """BASELINE C5 has 400 slices: the fp32 rounding of 4 x nz line transforms per pixel must stay below the 1e-4
    contract (measured 5e-5 at 400 slices).  1024^2 x 400 runs C3's grid at twice its depth; the 2048^2 stacks
    exercise every pass type of the 2048-point kernel with strong potentials; 501, 700 and 100 run the zero-padded
    convolution kernels (M = 1024, 2048, 256) at depth."""
    assert _deep().case(n, nz) < WAVE_TOL


def test_config_c5_grid_2048_400_slices(ps, orc):
    """BASELINE C5's grid and depth (2048^2, 400 slices) for one probe against the oracle slice loop (8 distinct
    potential slices cycled along z keep the synthesis of the input short; the loop still runs 400 different passes)."""
    assert _deep().case(2048, 400, distinct=8) < WAVE_TOL


def test_config_c3_64_probes_1024_200_slices_vs_oracle(ps, orc):
    """BASELINE C3's per-frame work exactly as bench.py runs it -- 1024^2 grid, 200 slices at full atom density,
    the 8 x 8 STEM probe grid of 03_manyprobes.py:16-28, so the launcher picks chunks of 16 probes per work item and the
    transposing kernel reuses t_k from registers across a chunk -- checked against the oracle for probes at the start
    and end of chunks and in the middle of one (the oracle costs ~8 s per probe here)."""
    from pyslice_amd.synthetic import synthetic_trajectory, stem_probe_grid
    n, nz = 1024, 200
    tr = synthetic_trajectory(n, nz, 1, seed=0)
    pp = [tuple(p) for p in stem_probe_grid(8)]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)[:, 0, :, :, 0]
    assert got.shape == (64, n, n)
    check = [0, 7, 15, 16, 37, 48, 62, 63]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, [pp[i] for i in check], workers=orc.usable_cores())["wavefunction_data"]
    for j, i in enumerate(check):
        assert rel_l2(got[i], want[j, 0, :, :, 0]) < WAVE_TOL, i
        assert ref_residual(got[i], want[j, 0, :, :, 0]) < RESID_TOL, i
    # every probe: norm conserved, and no two probes share a pattern
    k = np.fft.fftfreq(n, d=calc.dx)
    count = int((np.sqrt(k[:, None] ** 2 + k[None, :] ** 2) < 30e-3 / ps.wavelength(100e3)).sum())
    norms = (np.abs(got.astype(np.complex128)) ** 2).sum(axis=(1, 2))
    assert np.allclose(norms, count, rtol=2e-4)
    assert rel_l2(got[1], got[0]) > 1e-3 and rel_l2(got[62], got[63]) > 1e-3


def test_tacaw_1024_grid_k_window_256_frames_vs_oracle(ps, orc):
    """TACAW on C3's grid and frame count: 1024^2, T = 256 frames (wave-split register kernel), a 64 x 64 k-window so that
    the resident result stays small; against the oracle's time FFT of the oracle's own exit-wave spectra, cropped."""
    from pyslice_amd.synthetic import synthetic_trajectory
    n, nz, T = 1024, 2, 256
    tr = synthetic_trajectory(n, nz, T, density=0.02, seed=5)
    pp = [(40.0, 61.0)]
    calc = ps.MultisliceCalculator(progress=False, k_window=(64, 64))
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    tac = ps.TACAWData(wf)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp, workers=orc.usable_cores())["wavefunction_data"]
    win = want[:, :, n // 2 - 32:n // 2 + 32, n // 2 - 32:n // 2 + 32]
    assert rel_l2(npy(wf.wavefunction_data), win) < WAVE_TOL
    f, inten = orc.tacaw(win, wf.time)
    assert np.allclose(tac.frequencies, f)
    got = npy(tac.intensity)
    assert got.shape == (1, T, 64, 64)
    assert rel_l2(got, inten) < TACAW_TOL
    assert rel_l2(tac.spectrum(0), inten[0].sum(axis=(1, 2))) < TACAW_TOL


def test_randomised_shape_sweep(ps, orc):
    """40 random cases of tools/fuzz_parity.py (seed 11): grid shapes mixing the register, 2R^2, generic and Bluestein
    kernels, 1-12 slices, 1-4 probes, 1-2 frames, random k-windows; exit waves and windowed spectra against the oracle."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_parity.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    rng = np.random.default_rng(11)
    for c in range(40):
        cfg, err = fuzz.one(rng, max_pix=2 ** 20)
        assert err < WAVE_TOL, (cfg, err)


def test_randomised_potential_sweep(ps, orc):
    """40 random cases of tools/fuzz_potential.py (seed 5): grid shapes over every structure-factor / inverse-FFT path,
    1-3 species, atoms outside the box and outside every slice, one-pass and keep_potential engines."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzzp", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_potential.py"))
    fuzzp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzzp)
    rng = np.random.default_rng(5)
    for c in range(40):
        cfg, err = fuzzp.one(rng, max_pix=2 ** 18 if c % 4 else 2 ** 20)       # every fourth case may take the 513 .. 1100-point lengths
        assert err < POT_TOL, (cfg, err)


@pytest.mark.parametrize("two_tiles", [False, True])
@pytest.mark.parametrize("nx,ny,nz,n_atoms,batch", [(96, 80, 3, 1500, 1), (128, 128, 2, 2100, 3), (64, 250, 1, 400, 1), (256, 256, 4, 1100, 2),
                                                    (320, 200, 17, 9000, 1), (512, 512, 48, 21000, 1), (2048, 2048, 2, 4600, 1)])
def test_structure_factor_stream_kernel_dense_slices(ps, orc, nx, ny, nz, n_atoms, batch, two_tiles, monkeypatch):
    """From 128 atoms per (slice, species) on the potential takes structure_factor_stream_bf16_kernel (three-way bf16 split of
    every factor on the matrix instruction, f32 accumulation; measured 1.1e-7 .. 1.3e-7 of max|V|, the same as the f32 kernel;
    persistent, the rows of every bin
    padded to whole half-trips of 8, species flushed at half-trip boundaries): three species of which one is missing from a
    slice and one slice holds a single species, bin sizes that are and are not multiples of 8, several frames per build, odd grid
    lengths; and just below the threshold the tiled kernel on the same kind of input.  Transmission functions against the
    oracle's potential.  two_tiles: the kernel of the large grids (two tiles along kx per wave, species totals in the LDS,
    structure_factor_stream_bf16x2_kernel) forced onto the same inputs -- an odd number of tile columns (96, 320: the second tile of the
    last pair stores nothing), and 48 slices of 512 x 512 (48 work items for the 32 workgroups of an XCD: every workgroup runs several, the case in
    which the accumulators' zeroing between items needed its wait states)."""
    from pyslice_amd import _native
    if two_tiles and nx == 2048:
        pytest.skip("2048^2 takes the two-tile kernel by itself (512 tiles per slice and more)")
    if two_tiles:
        monkeypatch.setenv("MSL_DEBUG", "1")
        monkeypatch.setenv("MSL_SF_TWO_TILES", "1")
    from pyslice_amd.potentials import loadKirkland
    rng = np.random.default_rng(nx + n_atoms)
    dx, dy, dz = 0.1, 0.09, 0.5
    xs, ys, zs = np.arange(nx) * dx, np.arange(ny) * dy, np.arange(nz) * dz
    Z = rng.choice([5, 7, 14], size=n_atoms, p=[0.5, 0.4, 0.1]).astype(np.int32)
    eV = 100e3
    sig = orc.interaction_sigma(eV)
    frames = []
    for b in range(batch):
        pos = rng.random((n_atoms, 3)) * [nx * dx, ny * dy, nz * dz]
        if nz > 1:
            pos[(Z == 14) & (pos[:, 2] < 0.75), 2] += 0.6                # no Si in the first slice
            pos[(Z != 5) & (pos[:, 2] >= (nz - 1) * dz + 0.25 - dz / 2), 2] -= dz      # the last slice holds boron only
        frames.append(pos)
    eng = _native.Engine(nx, ny, nz, dx, dy, dz, orc.wavelength(eV), sig, n_probes=1, n_frames=batch, frame_batch=batch)
    eng.set_kirkland(loadKirkland())
    eng.set_slices(*orc.slice_edges(zs))
    if batch > 1:
        eng.build_potentials(np.stack(frames), Z, 2)
    else:
        eng.build_potential(frames[0], Z, 2)
    for b in range(batch):
        eng.select_batch_slot(b)
        V = orc.potential(xs, ys, zs, frames[b], Z)
        t = eng.transmission()
        err = np.abs(t - np.exp(1j * sig * np.moveaxis(V, 2, 0))).max() / (sig * np.abs(V).max())
        assert err < POT_TOL, (b, err)
    eng.close()


@pytest.mark.parametrize("nx,ny,nz,P", [(256, 256, 3, 700), (512, 512, 4, 70), (2048, 512, 4, 20), (1024, 512, 4, 33),
                                         (500, 360, 3, 40)])
def test_many_probes_per_launch(ps, orc, nx, ny, nz, P):
    """Several work items per workgroup, probe chunks with t_k reuse in registers, the 2048-point kernel's item loop
    with its re-parked propagator: every probe's spectrum against the oracle (tools/fuzz_many_probes.py)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fmp", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_many_probes.py"))
    fmp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fmp)
    assert fmp.case(nx, ny, nz, P) < WAVE_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(997, 64, 3, 100), (1200, 64, 3, 100)])
def test_item_loop_wraps_on_a_ragged_probe_chunk(ps, orc, monkeypatch, nx, ny, nz, P):
    """The work-item loop of rowTB2_pass_kernel (997 points: 513..1024, not smooth) and of rowTM2_pass_kernel (1200 = 2 x 25 x 24),
    which test_many_probes_per_launch does not reach, with a second item per workgroup and a ragged last probe chunk.
    Both kernels take the 64 lines of the long axis in 8 line blocks on 256 workgroups (one per CU).  choose_pchunk's cost
    ceil(8 ceil(100 / pc) / 256) pc is 4 for pc = 1 (800 items, 4 rounds), 2 (400, 2) and 4 (200, 1), more for every other chunk,
    and ties go to the larger: pc = 4, 200 items on 200 workgroups -- no second item, and 100 % 4 = 0.  So the chunk is set to 3
    (MSL_ROW_PCHUNK, read when the engine is created): 34 chunks, 8 x 34 = 272 items > 256 workgroups, so workgroups 0..15 take
    a second item, and 100 % 3 = 1: the last chunk of every line block holds one probe."""
    import importlib.util
    import os
    monkeypatch.setenv("MSL_DEBUG", "1")
    monkeypatch.setenv("MSL_ROW_PCHUNK", "3")
    spec = importlib.util.spec_from_file_location("fmp", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_many_probes.py"))
    fmp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fmp)
    assert fmp.case(nx, ny, nz, P) < WAVE_TOL


@pytest.mark.parametrize("nx,ny,nz,window,kbin,fb", [(256, 256, 3, None, (4, 4), 1), (256, 256, 4, (64, 96), (2, 8), 2),
                                                     (96, 80, 3, None, (3, 5), 1), (512, 512, 3, (128, 128), (4, 2), 3),
                                                     (1024, 256, 2, (256, 64), (16, 1), 1), (45, 63, 2, (15, 21), (5, 7), 2)])
def test_k_bin_is_a_block_sum_of_the_full_spectrum(ps, orc, nx, ny, nz, window, kbin, fb):
    """k_bin=(bx,by): every stored pixel is the (coherent) sum of bx x by neighbouring pixels of the fftshifted spectrum --
    the oracle's full array, cropped to the window, .reshape(.., wx/bx, bx, wy/by, by).sum().  Register and generic exit
    FFTs, with and without a k-window, with frame batching."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 3, ny=ny, density=0.05, seed=5 + nz)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(2).random((2, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, k_window=window, k_bin=kbin, frame_batch=fb)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    got = npy(wf.wavefunction_data)[..., 0]
    full = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"][..., 0]
    wx, wy = window if window else (nx, ny)
    x0, y0 = nx // 2 - wx // 2, ny // 2 - wy // 2
    win = full[:, :, x0:x0 + wx, y0:y0 + wy]
    want = win.reshape(2, 3, wx // kbin[0], kbin[0], wy // kbin[1], kbin[1]).sum(axis=(3, 5))
    assert got.shape == want.shape
    assert rel_l2(got, want) < WAVE_TOL
    kx, ky, _ = orc.wf_axes(nx, ny, 0.1, 3, tr.timestep)
    assert np.allclose(npy(wf.kxs), kx[x0:x0 + wx].reshape(-1, kbin[0]).mean(axis=1), rtol=1e-6, atol=1e-7)
    assert np.allclose(npy(wf.kys), ky[y0:y0 + wy].reshape(-1, kbin[1]).mean(axis=1), rtol=1e-6, atol=1e-7)
    # TACAW on the binned spectra = the oracle's time FFT of the binned array (three frames only: the intensity is the small
    # difference of nearly equal spectra, so the fp32 error of the spectra is amplified -- 1e-3 here)
    f, inten = orc.tacaw(want[..., None], wf.time)
    assert rel_l2(npy(ps.TACAWData(wf).intensity), inten) < 1e-3


def test_k_bin_argument_errors(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    with pytest.raises(ValueError):
        ps.MultisliceCalculator(progress=False, k_bin=(0, 2))
    with pytest.raises(ValueError):
        ps.MultisliceCalculator(progress=False, k_bin=(2, 2), cache=True)
    calc = ps.MultisliceCalculator(progress=False, k_bin=(3, 3))
    with pytest.raises(ValueError, match="multiple"):
        calc.setup(synthetic_trajectory(64, 2, 1, seed=1), aperture=30.0, voltage_eV=100e3)


@pytest.mark.parametrize("n,T,tile,P,fb,kbin", [(64, 40, 16, 2, 1, None), (64, 21, 8, 1, 4, (2, 2)), (96, 12, 12, 2, 1, None), (256, 9, 4, 3, 2, (4, 4))])
def test_streaming_tacaw_matches_the_full_transform(ps, orc, n, T, tile, P, fb, kbin):
    """stream_tile = Tt: the device holds a ring of Tt frames; run_streaming_tacaw() folds tile after tile into the
    time->frequency transform.  All bins: the oracle's intensity (tacaw_data.py:89-104); a frequency window: the same bins
    of it; total_diffraction: the oracle's sum over all frequencies, from the Parseval accumulators."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(n, 3, T, density=0.08, seed=31 + T)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(6).random((P, 2)) * [lx, ly]]
    full = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    if kbin:
        full = full[..., 0].reshape(P, T, n // kbin[0], kbin[0], n // kbin[1], kbin[1]).sum(axis=(3, 5))[..., None]
    f, inten = orc.tacaw(full, np.arange(T) * tr.timestep)
    calc = ps.MultisliceCalculator(progress=False, stream_tile=tile, frame_batch=fb, k_bin=kbin)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert calc._engine.n_frames == min(tile, T)
    with pytest.raises(RuntimeError):
        calc.run()
    tac = calc.run_streaming_tacaw()
    assert np.allclose(tac.frequencies, f)
    got = npy(tac.intensity)
    assert got.shape == inten.shape
    assert rel_l2(got, inten) < TACAW_TOL
    assert got[:, T // 2].max() == 0.0                                   # the DC bin (mean subtraction)
    assert rel_l2(tac.total_diffraction, inten.sum(axis=1)) < TACAW_TOL
    assert rel_l2(tac.spectrum(0), inten[0].sum(axis=(1, 2))) < TACAW_TOL
    # a frequency window keeps those bins only; the frequency-integrated pattern still covers every bin
    lo, hi = 0.0, 0.4 * f.max()
    sel = np.nonzero((f >= lo) & (f <= hi))[0]
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    tw = calc.run_streaming_tacaw(freq_window=(lo, hi))
    assert np.array_equal(tw.frequency_bins, sel) and np.allclose(tw.frequencies, f[sel])
    assert rel_l2(npy(tw.intensity), inten[:, sel]) < TACAW_TOL
    assert rel_l2(tw.total_diffraction, inten.sum(axis=1)) < TACAW_TOL
    assert rel_l2(tw.diffraction(P - 1), inten[P - 1][sel].sum(axis=0)) < TACAW_TOL


def test_streaming_fold_weak_bins_at_strong_pixels(ps):
    """The fold alone, on uploaded frames whose exact transform is known: a pixel with a time mean 1e5 times its thermal part
    (a Bragg spot or the central beam).  Every non-zero bin there is what is left after T large terms cancel; the fold
    subtracts the run's first frame before accumulating (msl_tacaw_stream_set_reference -- a constant offset only changes
    the u = 0 bin, which the mean subtraction of tacaw_data.py:94 zeroes), so the float32 accumulators hold the thermal part
    only.  Checked PER PIXEL at T = 256 and 1024 against the float64 DFT of the very same float32 frames."""
    from pyslice_amd import _native
    rng = np.random.default_rng(3)
    for T, ring in ((256, 32), (1024, 64)):
        nx = ny = 8
        eng = _native.Engine(nx, ny, 1, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=2, n_frames=ring)
        big = (rng.standard_normal((2, 1, nx, ny)) + 1j * rng.standard_normal((2, 1, nx, ny))) * 1e3
        big[:, :, ::2, ::3] = 0.0                                              # some pixels without a mean
        small = (rng.standard_normal((2, T, nx, ny)) + 1j * rng.standard_normal((2, T, nx, ny))) * 1e-2
        frames = (big + small).astype(np.complex64)                           # the data as the device sees it
        want = np.abs(np.fft.fftshift(np.fft.fft(frames.astype(np.complex128) - frames.astype(np.complex128).mean(axis=1, keepdims=True), axis=1), axes=1)) ** 2
        eng.tacaw_stream_begin(T, (np.arange(T) + (T + 1) // 2) % T)        # bins in fftshifted order, like the calculator
        for t0 in range(0, T, ring):
            for i in range(ring):
                eng.upload_frame(i, frames[:, t0 + i])
            if t0 == 0:
                eng.tacaw_stream_set_reference(slot=0)
            eng.tacaw_stream_push(0, ring, t0)
        total = eng.tacaw_stream_finish(True)
        got = eng.intensity().astype(np.float64)
        eng.close()
        assert got[:, T // 2].max() == 0.0
        err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)     # per (probe, pixel), over the frequency axis
        assert err.max() < 2e-5, (T, err.max())
        assert rel_l2(total, want.sum(axis=1)) < 2e-5            # T S2 - |S1|^2 in float64: 1e11 cancels to 1e1


def test_streaming_tacaw_c5_grid_window_and_bin(ps, orc):
    """BASELINE C5's grid (2048^2) with the k-window and bin DESIGN picks for it (window 512 x 512, bin 4 x 4), a shallow stack
    so that the oracle stays affordable: streamed TACAW of 6 frames against the oracle's transform of its own binned window."""
    from pyslice_amd.synthetic import synthetic_trajectory
    n, T = 2048, 6
    tr = synthetic_trajectory(n, 2, T, density=0.01, seed=77)
    pp = [(101.0, 99.0), (60.0, 140.0)]
    calc = ps.MultisliceCalculator(progress=False, stream_tile=4, k_window=(512, 512), k_bin=(4, 4))
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    tac = calc.run_streaming_tacaw()
    full = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"][..., 0]
    win = full[:, :, n // 2 - 256:n // 2 + 256, n // 2 - 256:n // 2 + 256].reshape(2, T, 128, 4, 128, 4).sum(axis=(3, 5))
    f, inten = orc.tacaw(win[..., None], np.arange(T) * tr.timestep)
    assert npy(tac.intensity).shape == (2, T, 128, 128)
    assert rel_l2(npy(tac.intensity), inten) < TACAW_TOL
    assert rel_l2(tac.total_diffraction, inten.sum(axis=1)) < TACAW_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(501, 491, 5, 3), (500, 500, 4, 2), (33, 128, 3, 2), (129, 272, 4, 2),
                                        (100, 400, 3, 3), (512, 300, 4, 2), (349, 1024, 3, 1), (271, 257, 2, 2),
                                        (491, 501, 1, 2), (360, 448, 2, 70), (192, 180, 3, 2), (200, 191, 4, 2)])
def test_any_length_register_kernel_matches_oracle(ps, orc, nx, ny, nz, P):
    """Lines of any length up to 512 run on the register FFTs (rowTB_pass_kernel: M = 256 for n <= 128, M = 1024 for
    192 <= n <= 512 and for every non-smooth n in between), the propagation A = ifft.P.fft as ONE zero-padded cyclic convolution
    of length M (two FFTs): the reference's own 501 x 491 grid (src/unittests/00_probe.py:7-8) in both orientations, the
    boundaries of the length ranges, line counts that are not multiples of 16, mixes with the power-of-two and generic kernels,
    many probes, odd and even depths."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 2, ny=ny, density=0.04, seed=nx + ny)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(9).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    chk = list(range(P)) if P <= 3 else [0, P // 2, P - 1]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, [pp[i] for i in chk])["wavefunction_data"]
    assert rel_l2(got[chk], want) < WAVE_TOL
    assert ref_residual(got[chk], want) < RESID_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(997, 600, 3, 2), (700, 700, 4, 1), (513, 1000, 2, 2), (1021, 576, 3, 1),
                                        (641, 333, 3, 2), (768, 1024, 2, 1)])
def test_lengths_513_to_1024_on_the_2048_point_wave_fft(ps, orc, nx, ny, nz, P):
    """Lines of 513..1024 points run on the wave-per-line 2048-point register FFT (rowTB2_pass_kernel, the zero-padded cyclic
    convolution of length 2048): primes, range ends, smooth lengths (600, 768), line counts that are not multiples of 8, mixes
    with the 1024-point kernel and a power-of-two direction."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.02, seed=nx + 3 * ny)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(10).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(600, 600, 4, 3), (360, 480, 3, 2), (144, 225, 3, 2), (960, 320, 2, 1), (900, 729, 3, 1),
                                        (500, 1024, 3, 2), (250, 810, 2, 2), (648, 405, 3, 1), (768, 150, 2, 2), (625, 997, 2, 1),
                                        (1000, 600, 3, 2), (1500, 972, 2, 1), (1728, 1200, 2, 1), (1250, 1024, 3, 1), (1080, 1536, 2, 2),
                                        (1600, 1458, 2, 1), (1620, 2048, 2, 1), (1152, 1011, 3, 1)])
def test_smooth_lengths_on_the_mixed_radix_pass(ps, orc, nx, ny, nz, P):
    """Lines of a smooth length A * B (A, B <= 32) run on rowTM_pass_kernel, the direct mixed-radix four-step transform
    (rowtm_pass.h): balanced and lopsided factorisations, radix 3 / 5 / 4 / 2 register transforms, groups of 16 and of 32 lanes, the
    kernels that spill a few registers (900, 729, 960), line counts that are not multiples of 16, odd and even depths, and mixes
    with a power-of-two axis (1024), a convolution axis (997) and the small-group kernels (150, 144).  Lengths 2 A * B up to 1728 run
    on rowTM2_pass_kernel (one wave per line, radix-2 step across lane pairs): next to each other, to the A * B kernels, to 1024- and
    2048-point axes and to a convolution axis (1011), line counts that are not multiples of 8."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.02, seed=nx + 3 * ny)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(12).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(700, 700, 4, 3), (448, 336, 3, 2), (196, 147, 3, 2), (896, 504, 2, 1), (784, 840, 2, 1),
                                        (175, 189, 3, 2), (140, 135, 3, 2), (441, 420, 3, 2), (567, 997, 2, 1), (1400, 1120, 2, 1), (1680, 1568, 2, 1),
                                        (1050, 630, 3, 2), (1512, 1024, 2, 1), (210, 1176, 2, 2)])
def test_lengths_with_a_factor_7_on_the_mixed_radix_pass(ps, orc, nx, ny, nz, P):
    """7-smooth line lengths (mixed radix 3, 5, 7) on the same direct passes with the radix-7 register butterfly
    (fft_regs.h: dif7_level): the factor 7 in the lane count, in the register count or in both (441, 784), 7 x 7 = 49 nowhere (factors
    <= 32), groups of 16 lanes (196) and of 32, the kernels that spill a few registers (784, 896; 1512, 1568, 1680), the 2 A B form on one
    wave per line (1050 .. 1680), next to 5-smooth, power-of-two and convolution axes, line counts that are not multiples of the tile."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.02, seed=nx + 5 * ny)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(13).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL


@pytest.mark.parametrize("nz", [3, 2])
def test_transmission_functions_2048_grid(ps, orc, nz):
    """exp(i sigma V) on the C5 grid straight against the oracle: quadrant structure factor, half-spectrum inverse transform on the
    2048-point wave FFT (ifftTW_kernel), x-pass slices kept transposed and restored by the download; odd and even depths."""
    from pyslice_amd import _native
    from pyslice_amd.potentials import loadKirkland, slice_edges
    rng = np.random.default_rng(3 + nz)
    n, dx, dz, na = 2048, 0.1, 0.5, 300
    xs, zs = np.arange(n) * dx, np.arange(nz) * dz
    pos = rng.random((na, 3)) * [n * dx, n * dx, nz * dz]
    Z = rng.choice([6, 14, 79], size=na).astype(np.int32)
    sig = orc.interaction_sigma(100e3)
    want = np.exp(1j * sig * np.moveaxis(orc.potential(xs, xs, zs, pos, Z), 2, 0))
    eng = _native.Engine(n, n, nz, dx, dx, dz, orc.wavelength(100e3), sig, n_probes=1, n_frames=0)
    eng.set_kirkland(loadKirkland())
    eng.set_slices(*slice_edges(zs))
    eng.build_potential(pos, Z, 2)
    got = np.asarray(eng.transmission())
    eng.close()
    assert np.abs(got - want).max() < 1e-5


@pytest.mark.parametrize("nx,ny,nz,P,mode", [(1100, 1030, 3, 2, "two_waves"), (1025, 512, 2, 1, "two_waves"), (2047, 1200, 2, 1, "two_waves"),
                                             (1500, 1029, 4, 3, "two_waves"), (1100, 1030, 2, 1, "generic")])
def test_lengths_1025_to_2047(ps, orc, nx, ny, nz, P, mode, monkeypatch):
    """Lines of 1025..2047 points: cyclic convolution of length 4096 on pairs of 2048-point wave FFTs, the two branches of the
    radix-2 step on two waves (rowTC2_pass_kernel), and the generic LDS kernels in the two-pass loop as the cross-check
    (MSL_DEBUG + MSL_NO_CONV4096); next to a 513..1024-point and a 512-point axis, odd and even depths."""
    from pyslice_amd.synthetic import synthetic_trajectory
    if mode == "generic":
        monkeypatch.setenv("MSL_DEBUG", "1")
        monkeypatch.setenv("MSL_NO_CONV4096", "1")
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.01, seed=nx + ny)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(3).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL


@pytest.mark.parametrize("nx,ny,nz,P", [(2048, 2048, 3, 1), (2048, 2048, 4, 2), (2048, 512, 3, 2), (2048, 2048, 1, 1)])
def test_2048_point_wave_per_line_kernel_matches_oracle(ps, orc, nx, ny, nz, P, monkeypatch):
    """2048-point lines on fft2048_wave (one wave per line, paired-lines layout between two such passes; a 2048 x 512 grid
    alternates with the 512-point kernel through the natural layout); odd and even depths."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, nz, 1, ny=ny, density=0.004, seed=nz)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(12).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(got, want) < WAVE_TOL
    assert ref_residual(got, want) < RESID_TOL


def test_any_length_register_kernel_deep_stack_and_generic_cross_check(ps, orc, monkeypatch):
    """501 x 491, 100 slices: error growth of the chirp-z passes (8 length-1024 FFTs per line and pass) stays inside the
    contract, and the generic LDS kernels (MSL_NO_BLUESTEIN_REG) give the same exit waves."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(501, 100, 1, ny=491, density=0.03, seed=3)
    pp = [(20.0, 30.0)]
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("MSL_DEBUG", "1")
            monkeypatch.setenv("MSL_NO_BLUESTEIN_REG", "1")
        calc = ps.MultisliceCalculator(progress=False)
        calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        outs.append(npy(calc.run().wavefunction_data))
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    assert rel_l2(outs[0], want) < WAVE_TOL and rel_l2(outs[1], want) < WAVE_TOL
    assert rel_l2(outs[0], outs[1]) < 5e-5


def test_k_window_argument_errors(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(32, 2, 1, density=0.05, seed=1)
    with pytest.raises(ValueError):
        ps.MultisliceCalculator(progress=False, k_window=(0, 8))
    with pytest.raises(ValueError):
        ps.MultisliceCalculator(progress=False, k_window=(8, 8), cache=True)
    calc = ps.MultisliceCalculator(progress=False, k_window=(64, 8))
    with pytest.raises(ValueError):
        calc.setup(tr)                           # window larger than the 32 x 32 grid


def test_oracle_parity_prime_grid(ps, orc):
    """Grid lengths with large prime factors (101 x 97, like the reference's 501 x 491 probe test grid) take the
    Bluestein path; potential, probes and slice loop must still match the oracle."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(101, 8, 1, ny=97, density=0.15, seed=6)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    assert (len(xs), len(ys), len(zs)) == (101, 97, 8)
    pp = [(lx / 2, ly / 2), (1.3, 7.7)]
    V = orc.potential(xs, ys, zs, tr.positions[0], tr.atom_types)
    pr = orc.batched_probes(orc.probe_array(xs, ys, 30.0, 100e3), xs, ys, pp)
    ex = orc.propagate(pr, V, xs, ys, zs, 100e3)
    pot = ps.Potential(xs, ys, zs, tr.positions[0], list(tr.atom_types))
    assert np.abs(V - npy(pot.array)).max() / np.abs(V).max() < POT_TOL
    probes = ps.create_batched_probes(ps.Probe(xs, ys, 30.0, 100e3), pp)
    assert rel_l2(npy(probes.array), pr) < 1e-5
    gex = npy(ps.Propagate(probes, pot))
    assert rel_l2(gex, ex) < WAVE_TOL
    assert ref_residual(gex, ex) < RESID_TOL


def test_oracle_parity_512_100slices(ps, orc):
    """BASELINE config C2 grid (512^2, 100 slices), one frame; lower atom density keeps the oracle to seconds."""
    V, Vg, ex, gex = _oracle_case(ps, orc, 512, 100, 1, 30.0, density=0.02, seed=4)
    assert np.abs(V - Vg).max() / np.abs(V).max() < POT_TOL
    assert rel_l2(gex, ex) < WAVE_TOL
    assert ref_residual(gex, ex) < RESID_TOL


# ------------------------------------------------------------------ known answers / size-independent properties
def test_k1_vacuum_plane_wave(ps):
    from pyslice_amd import _native
    n, nz = 256, 20
    eng = _native.Engine(n, n, nz, 0.1, 0.1, 0.5, 0.0370144, 9.24396e-4, n_probes=2, n_frames=1)
    eng.upload_potential(np.zeros((nz, n, n), dtype=np.float32))
    eng.set_probes(0.0, [(1.0, 2.0), (3.0, 4.0)])
    eng.propagate_frame(0)
    wf = eng.wavefunction()
    for p in range(2):
        d = wf[p, 0].copy()
        assert abs(d[n // 2, n // 2] - n * n) < 1e-3 * n * n
        d[n // 2, n // 2] = 0
        assert np.abs(d).max() < 1e-3 * n
    eng.close()


def test_k3_single_slice_is_transmission_times_probe(ps, orc):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 1, 1, density=0.3, seed=9)
    xs, ys, zs, *_ = ps.gridFromTrajectory(tr)
    assert len(zs) == 1
    pot = ps.Potential(xs, ys, zs, tr.positions[0], list(tr.atom_types))
    pr = ps.Probe(xs, ys, 30.0, 100e3)
    ex = npy(ps.Propagate(pr, pot))
    V = npy(pot.array)[:, :, 0]
    want = np.exp(1j * orc.interaction_sigma(100e3) * V) * npy(ps.Probe(xs, ys, 30.0, 100e3).array)
    assert rel_l2(ex, want) < 1e-5


def test_k4_potential_integral_on_device(ps):
    """K4, no oracle: sum_xy V[:,:,s] dx^2 dy^2 = sum over the atoms of slice s of f_Z(0), with
    f_Z(0) = sum_i a_i / b_i + sum_i c_i straight from the Kirkland table -- the DC bin of every slice."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, 1, ny=80, density=0.08, seed=12)
    xs, ys, zs, *_ = ps.gridFromTrajectory(tr)
    pot = ps.Potential(xs, ys, zs, tr.positions[0], list(tr.atom_types))
    V = npy(pot.array)
    table = ps.loadKirkland()                                           # (103, 3, 4): a, b, c, d
    f0 = {int(Z): float((table[Z - 1][:, 0] / table[Z - 1][:, 1]).sum() + table[Z - 1][:, 2].sum()) for Z in set(tr.atom_types)}
    dx, dy, dz = xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]
    lo = np.r_[0.0, zs[1:] - dz / 2]
    hi = np.r_[zs[:-1] + dz / 2, zs[-1] + dz]
    z = tr.positions[0][:, 2]
    for s_ in range(len(zs)):
        m = (z >= lo[s_]) & (z < hi[s_])
        want = sum(f0[int(Z)] for Z in np.asarray(tr.atom_types)[m])
        got = float(V[:, :, s_].astype(np.float64).sum()) * dx ** 2 * dy ** 2
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (s_, got, want)


def test_k6_probe_peak_position_on_device(ps):
    """K6 / quirk Q3, no oracle: the probe 'at p' of create_batched_probes peaks at (L/2 - p) mod L."""
    nx, ny, dx, dy = 128, 96, 0.1, 0.12
    xs, ys = np.arange(nx) * dx, np.arange(ny) * dy
    pp = [(1.0, 2.0), (6.4, 5.76), (11.3, 0.5), (0.0, 9.0)]
    arr = npy(ps.create_batched_probes(ps.Probe(xs, ys, 30.0, 100e3), pp).array)
    for a, (px, py) in zip(arr, pp):
        i, j = np.unravel_index(np.argmax(np.abs(a)), a.shape)
        ex, ey = ((nx // 2) * dx - px) % (nx * dx), ((ny // 2) * dy - py) % (ny * dy)
        assert min(abs(i * dx - ex), nx * dx - abs(i * dx - ex)) <= dx
        assert min(abs(j * dy - ey), ny * dy - abs(j * dy - ey)) <= dy


def test_k2_norm_conserved_full_size(ps):
    """BASELINE full grid (1024^2, 200 slices): |t|=|P|=1, so sum|Psi_k|^2 = nx*ny * (aperture pixel count)."""
    from pyslice_amd.synthetic import synthetic_trajectory, stem_probe_grid
    n, nz = 1024, 200
    tr = synthetic_trajectory(n, nz, 1, seed=0)
    pp = stem_probe_grid(2)
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=[tuple(p) for p in pp])
    wf = calc.run()
    data = npy(wf.wavefunction_data)[..., 0]
    assert data.shape == (4, 1, n, n)
    k = np.fft.fftfreq(n, d=calc.dx)
    count = int((np.sqrt(k[:, None] ** 2 + k[None, :] ** 2) < 30e-3 / ps.wavelength(100e3)).sum())
    norms = (np.abs(data.astype(np.complex128)) ** 2).sum(axis=(2, 3))[:, 0]
    assert np.allclose(norms, count, rtol=2e-4)        # sum|psi0|^2 = count/(nx ny) (quirk Q4), FFT gains nx ny
    # different probe positions see different columns of atoms -> patterns differ, norms agree
    assert rel_l2(data[0], data[3]) > 1e-3


def test_errors_match_reference_types(ps):
    with pytest.raises(ValueError):
        ps.Trajectory(np.array([5, 7]), np.zeros((1, 2, 2)), np.zeros((1, 2, 3)), np.eye(3), 0.005)
    with pytest.raises(NotImplementedError):
        ps.MultisliceCalculator(force_cpu=True)


# ------------------------------------------------------------------ edge cases (empty / ragged / out-of-range inputs)
def test_edge_atoms_outside_every_slice_give_vacuum(ps, orc):
    xs = np.linspace(0, 6.4, 64, endpoint=False); zs = np.linspace(0, 2.0, 4, endpoint=False)
    pos = np.array([[1.0, 1.0, -0.2], [2.0, 2.0, 9.0]])           # z<0 and z beyond the last slice: dropped (Q7)
    pot = ps.Potential(xs, xs, zs, pos, [5, 7])
    assert np.abs(npy(pot.array)).max() == 0.0
    want = orc.propagate(orc.probe_array(xs, xs, 30.0, 100e3)[None], np.zeros((64, 64, 4)), xs, xs, zs, 100e3)[0]
    got = npy(ps.Propagate(ps.Probe(xs, xs, 30.0, 100e3), pot))
    assert rel_l2(got, want) < 1e-5


def test_edge_single_atom_and_out_of_box_probe_positions(ps, orc):
    xs = np.linspace(0, 6.4, 64, endpoint=False); ys = np.linspace(0, 4.8, 48, endpoint=False)
    zs = np.linspace(0, 1.5, 3, endpoint=False)
    pos = np.array([[6.39, 0.01, 0.74]])
    V = orc.potential(xs, ys, zs, pos, np.array([79]))
    pot = ps.Potential(xs, ys, zs, pos, ["Au"])
    assert np.abs(V - npy(pot.array)).max() / np.abs(V).max() < POT_TOL
    pp = [(-3.0, 100.0), (6.4, 4.8), (0.0, -0.05)]                # outside the box: the ramp simply wraps
    pr = orc.batched_probes(orc.probe_array(xs, ys, 30.0, 200e3), xs, ys, pp)
    ex = orc.propagate(pr, V, xs, ys, zs, 200e3)
    got = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(xs, ys, 30.0, 200e3), pp), pot))
    assert rel_l2(got, ex) < WAVE_TOL


def test_edge_many_probes_small_grid_and_two_frames(ps, orc):
    """900 probes on a 32^2 grid (the notebook's 30x30 STEM raster shape), T = 2 (the TACAW minimum)."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(32, 3, 2, density=0.3, seed=8)
    pp = ps.probe_grid([0.3, 2.9], [0.2, 3.0], 30, 30)
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=[tuple(p) for p in pp])
    wf = calc.run()
    data = npy(wf.wavefunction_data)
    assert data.shape == (900, 2, 32, 32, 1)
    sel = [0, 17, 449, 899]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, [tuple(pp[i]) for i in sel])["wavefunction_data"]
    assert rel_l2(data[sel], want) < WAVE_TOL
    tac = ps.TACAWData(wf)
    f, inten = orc.tacaw(want, wf.time)
    assert np.allclose(tac.frequencies, f)
    assert rel_l2(npy(tac.intensity)[sel], inten) < TACAW_TOL


def test_edge_bad_arguments_raise_value_errors(ps):
    from pyslice_amd import _native
    eng = _native.Engine(64, 64, 2, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=2, n_frames=1)
    with pytest.raises(ValueError):
        eng.set_probes(30.0, [(1.0, 1.0)])                       # wrong probe count
    with pytest.raises(ValueError):
        eng.build_potential(np.zeros((3, 2)), np.array([5, 5, 5]))
    eng.set_kirkland(ps.loadKirkland()); eng.set_slices(np.array([0.0, 0.25]), np.array([0.25, 1.0]))
    with pytest.raises(ValueError):
        eng.build_potential(np.zeros((1, 3)), np.array([0]))      # Z out of 1..103
    with pytest.raises(RuntimeError):
        eng.propagate()                                           # no probes / potential yet
    with pytest.raises(ValueError):
        eng.propagate_frame(5)
    eng.close()


# ------------------------------------------------------------------ BASELINE configs / domain known answers
def test_config_c2_shape_512_100slices_64frames(ps, orc):
    """BASELINE configs[1]: single probe, 64 MD frames, 512^2 grid, 100 slices on one GPU.  All 64 frames run on the
    device; the last frame is validated against the oracle at full atom density (the oracle needs ~15 s per frame)."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(512, 100, 64, seed=2)
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64")
    calc.setup(tr, aperture=30.0, voltage_eV=100e3)
    assert (calc.nx, calc.ny, calc.nz, calc.n_probes, calc.n_frames) == (512, 512, 100, 1, 64)
    wf = calc.run()
    data = npy(wf.wavefunction_data)
    assert data.shape == (1, 64, 512, 512, 1)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, frames=[63])["wavefunction_data"]
    assert rel_l2(data[:, 63:64], want) < WAVE_TOL
    assert ref_residual(data[:, 63:64], want) < RESID_TOL
    # frames differ (the atoms move) but every frame conserves the norm (K2)
    norms = (np.abs(data[0, :, :, :, 0].astype(np.complex128)) ** 2).sum(axis=(1, 2))
    assert np.allclose(norms, norms[0], rtol=2e-4)
    assert rel_l2(data[0, 0], data[0, 32]) > 1e-3


def test_k5_tacaw_peaks_at_phonon_frequencies(ps):
    """K5: atoms oscillating at 10/25/40 THz (pyslice_amd.synthetic) put the TACAW spectrum's weight into the
    +-10, +-25, +-40 THz bins and nothing into the DC bin."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 4, 40, density=0.25, seed=5)         # T*dt = 0.2 ps -> 5 THz bins
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=0.0, voltage_eV=100e3)
    tac = ps.TACAWData(calc.run())
    f = tac.frequencies
    spec = tac.spectrum(0)
    assert np.isclose(f[1] - f[0], 5.0)
    on = np.isin(np.round(np.abs(f)).astype(int), [10, 25, 40])
    assert spec[np.argmin(np.abs(f))] == 0.0
    assert spec[on].sum() > 0.8 * spec.sum()          # the rest is multi-phonon (sum and difference) weight
    assert spec[on].min() > 20 * np.median(spec[~on])


def test_frame_cache_format_and_resume(ps, golden, tmp_path, monkeypatch):
    """Opt-in frame cache: files named and shaped like the reference's (frame_<i>.npy, (P,nx,ny,1,1) complex128,
    calculators.py:173, 279, 311); a second run loads them instead of computing (resume)."""
    g = golden("g7_calculator_64")
    pos = g["positions"]
    tr = ps.Trajectory(g["Z"], pos, np.zeros_like(pos), g["box"], 0.005)
    pp = [tuple(p) for p in g["probe_positions"]]
    monkeypatch.chdir(tmp_path)
    calc = ps.MultisliceCalculator(progress=False, cache=True)
    calc.setup(tr, aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), probe_positions=pp)
    wf1 = npy(calc.run().wavefunction_data)
    assert (calc.frames_computed, calc.frames_cached) == (pos.shape[0], 0)
    files = sorted(calc.output_dir.glob("frame_*.npy"))
    assert len(files) == pos.shape[0] and str(calc.output_dir).startswith("psi_data/torch_")
    f0 = np.load(calc.output_dir / "frame_0.npy")
    assert f0.shape == (len(pp), 64, 64, 1, 1) and f0.dtype == np.complex128
    assert rel_l2(f0[:, :, :, 0, 0], g["wavefunction_data"][:, 0, :, :, 0]) < WAVE_TOL
    calc2 = ps.MultisliceCalculator(progress=False, cache=True)
    calc2.setup(tr, aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), probe_positions=pp)
    wf2 = npy(calc2.run().wavefunction_data)
    assert (calc2.frames_computed, calc2.frames_cached) == (0, pos.shape[0])
    assert np.array_equal(wf1, wf2)
    # without cache=True nothing is written
    monkeypatch.chdir(tmp_path / "psi_data")
    calc3 = ps.MultisliceCalculator(progress=False)
    calc3.setup(tr, aperture=float(g["aperture"]), voltage_eV=float(g["eV"]), probe_positions=pp)
    calc3.run()
    assert not (tmp_path / "psi_data" / "psi_data").exists()


def test_frame_cache_shared_with_reference(ps, golden, tmp_path, monkeypatch):
    """A psi_data/ directory written by the REFERENCE (g11: its directory name and its frame_0.npy) is found and
    resumed from by the build, and the frames the build writes have the reference's name, shape, dtype and values."""
    g = golden("g11_cache")
    monkeypatch.chdir(tmp_path)
    for c in ("a", "b"):
        pp = [tuple(float(v) for v in p) for p in g[f"probe_positions_{c}"]] if bool(g[f"has_positions_{c}"]) else None
        pos = g[f"positions_{c}"]
        tr = ps.Trajectory(g[f"Z_{c}"], pos, np.zeros_like(pos), g[f"box_{c}"], 0.005)
        calc = ps.MultisliceCalculator(progress=False, cache=True)
        calc.setup(tr, aperture=float(g[f"aperture_{c}"]), voltage_eV=float(g[f"eV_{c}"]), probe_positions=pp)
        assert calc.output_dir.name == str(g[f"dir_name_{c}"])
        np.save(calc.output_dir / "frame_0.npy", g[f"frame0_{c}"])           # the reference's own cache file
        wf = npy(calc.run().wavefunction_data)
        assert (calc.frames_computed, calc.frames_cached) == (pos.shape[0] - 1, 1)
        assert rel_l2(wf[:, 0], g[f"wavefunction_frame0_{c}"]) < 1e-6           # loaded (complex64 on the device)
        f1 = np.load(calc.output_dir / "frame_1.npy")
        assert f1.shape == g[f"frame0_{c}"].shape and f1.dtype == np.complex128


def test_g10_probe_defocus(ps, golden):
    """Probe.defocus (reference multislice.py:183-190) for dz > 0 and dz < 0 -- the reference defocuses by +|dz| for
    either sign (it divides by P(dz<0)); 07_defocus.py's 1000 A included."""
    g = golden("g10_defocus")
    for tag in ("64", "96x80"):
        xs, ys = g[f"xs_{tag}"], g[f"ys_{tag}"]
        for dz in g["dz"]:
            pr = ps.Probe(xs, ys, float(g["mrad"]), float(g["eV"]))
            pr.defocus(float(dz))
            assert rel_l2(npy(pr.array), g[f"defocus_{tag}_{dz:g}"]) < 5e-6
    pr = ps.Probe(g["xs_64"], g["ys_64"], 30.0, 100e3)
    before = npy(pr.array).copy()
    pr.defocus(0)
    assert np.array_equal(npy(pr.array), before)


@pytest.mark.parametrize("T", [2, 3, 33, 40, 100, 101, 128, 129, 255, 256, 257, 500, 512])
@pytest.mark.parametrize("shape", [(8, 8), (6, 8), (7, 9), (5, 14)])
def test_tacaw_any_frame_count_on_the_register_kernel(ps, T, shape):
    """The reference transforms whatever frame count the trajectory has (tacaw_data.py:94-96; 100 frames in its notebook,
    example.ipynb:578).  Every T <= 512 runs a register kernel -- the mixed-radix ones for the smooth counts (per lane from 16
    to 128: 40, 100, 128 here; split over waves above: 256, 500, 512; all of them in the next test), else chirp-z
    (time_cz_kernel: M = 256 for T <= 128 on 32- or 16-pixel tiles, M = 1024 above: 2, 3, 33, 101, 129, 255, 257): against the float64 transform of the same float32 frames, per pixel -- some
    pixels with a time mean 1e4 times their thermal part (the kernel subtracts the line's first sample instead of the mean) --
    and against the generic LDS kernel.  Pixel counts that are multiples of the tile, ragged (48, 70) and odd (63: the reference's
    own 501 x 491 test grid has an odd pixel count)."""
    from pyslice_amd import _native
    rng = np.random.default_rng(T)
    nx, ny = shape
    eng = _native.Engine(nx, ny, 1, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=3, n_frames=T)
    big = (rng.standard_normal((3, 1, nx, ny)) + 1j * rng.standard_normal((3, 1, nx, ny))) * 1e2
    big[:, :, ::2, ::3] = 0.0
    small = (rng.standard_normal((3, T, nx, ny)) + 1j * rng.standard_normal((3, T, nx, ny))) * 1e-2
    frames = (big + small).astype(np.complex64)
    f64 = frames.astype(np.complex128)
    want = np.abs(np.fft.fftshift(np.fft.fft(f64 - f64.mean(axis=1, keepdims=True), axis=1), axes=1)) ** 2
    for t in range(T):
        eng.upload_frame(t, frames[:, t])
    eng.tacaw()
    got = eng.intensity().astype(np.float64)
    assert got.shape == want.shape
    assert got[:, T // 2].max() == 0.0
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert err.max() < 5e-5, (T, err.max())
    os.environ["MSL_DEBUG"] = os.environ["MSL_TACAW_GENERIC"] = "1"
    try:
        eng.tacaw()
        gen = eng.intensity().astype(np.float64)
    finally:
        del os.environ["MSL_TACAW_GENERIC"], os.environ["MSL_DEBUG"]
    eng.close()
    weak = big[:, 0] == 0
    assert rel_l2(got.transpose(0, 2, 3, 1)[weak], gen.transpose(0, 2, 3, 1)[weak]) < 1e-5
    # (the generic kernel subtracts the line's first sample too: it holds per pixel at the strong-mean pixels as well)
    gerr = np.linalg.norm(gen - want, axis=1) / np.linalg.norm(want, axis=1)
    assert gerr.max() < 5e-5, (T, gerr.max())


@pytest.mark.parametrize("shape", [(8, 8), (6, 8)])
def test_tacaw_1024_frames_on_the_four_step_kernel(ps, shape):
    """T = 1024 (BASELINE C5's frame count) when the whole (P, T, nx, ny) array is resident: the 32 x 32 four-step column kernel
    (col_pass_kernel, COL_INTENSITY; pixel counts that are multiples of 16; the default only for images above 4.1 M pixels, where
    the wave-split kernel's 32-bit row offsets end), per pixel against the float64 transform, strong-mean pixels included, and
    against the wave-split kernel."""
    from pyslice_amd import _native
    T = 1024
    rng = np.random.default_rng(7)
    nx, ny = shape
    eng = _native.Engine(nx, ny, 1, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=2, n_frames=T)
    big = (rng.standard_normal((2, 1, nx, ny)) + 1j * rng.standard_normal((2, 1, nx, ny))) * 1e2
    big[:, :, ::2, ::3] = 0.0
    small = (rng.standard_normal((2, T, nx, ny)) + 1j * rng.standard_normal((2, T, nx, ny))) * 1e-2
    frames = (big + small).astype(np.complex64)
    f64 = frames.astype(np.complex128)
    want = np.abs(np.fft.fftshift(np.fft.fft(f64 - f64.mean(axis=1, keepdims=True), axis=1), axes=1)) ** 2
    for t in range(T):
        eng.upload_frame(t, frames[:, t])
    os.environ["MSL_DEBUG"] = os.environ["MSL_TACAW_FOURSTEP"] = "1"      # (images this small take the wave-split kernel by default)
    try:
        eng.tacaw()
    finally:
        del os.environ["MSL_TACAW_FOURSTEP"], os.environ["MSL_DEBUG"]
    got = eng.intensity().astype(np.float64)
    eng.tacaw()
    split = eng.intensity().astype(np.float64)
    eng.close()
    assert got[:, T // 2].max() == 0.0
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert err.max() < 5e-5, err.max()
    assert not np.array_equal(got, split) and rel_l2(got, split) < 2e-5


@pytest.mark.parametrize("T", [100, 125, 200, 300, 375, 486, 500, 101, 1000, 1024])
def test_tacaw_many_tiles_per_workgroup(ps, T):
    """The time kernels are persistent: a workgroup walks over many tiles with the next tile's samples prefetched in registers
    (rolling prefetch, alternating exchange buffers, the last tile prefetching itself).  The small parity cases give every
    workgroup ONE tile; here 2 probes x 300 007 pixels (odd: unvectorised chirp-z path, ragged last tile everywhere) make 2 300 to
    18 800 tiles for at most 1 024 workgroups -- one frame count per kernel family: per-lane (100; 125: partial prefetch), two
    blocks per wave (200 = 2 x 100, 300 = 4 x 75, 500 = 4 x 125, 1000 = 8 x 125, 1024), one block per wave (375 = 3 x 125,
    486 = 6 x 81), chirp-z (101).  Checked on 3 000 random pixels per probe against the float64 transform of the same float32
    samples (strong-mean pixels included) and on ALL pixels through Parseval: sum_w I[w] = T sum_t |x_t - <x>|^2."""
    import torch
    from pyslice_amd import _native
    P, npix = 2, 300007
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T)
    big = torch.randn((P, 1, npix, 2), generator=g, device=dev) * 1e2
    big[:, :, ::3] = 0.0
    src = torch.view_as_complex((big + torch.randn((P, T, npix, 2), generator=g, device=dev) * 1e-2).contiguous())
    dst = torch.full((P, T, npix), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()                                           # (torch's stream filled src / dst; the library has its own)
    eng = _native.Engine(2, 2, 1, 1.0, 1.0, 1.0, 1.0, 0.0, n_probes=1, n_frames=0, device=0)
    eng.tacaw(src.data_ptr(), dst.data_ptr(), P, T, npix)
    eng.synchronize()
    eng.close()
    assert float(dst.min()) >= 0.0                                     # every element was written
    assert float(dst[:, T // 2].max()) == 0.0
    x64 = src.to(torch.complex128)
    x64 = x64 - x64.mean(dim=1, keepdim=True)
    want_sum = T * (x64.abs() ** 2).sum(dim=1)
    got_sum = dst.to(torch.float64).sum(dim=1)
    assert float(((got_sum - want_sum).abs() / want_sum).max()) < 2e-5
    pick = torch.from_numpy(np.random.default_rng(T).choice(npix, 3000, replace=False)).to(dev)
    pick[:4] = torch.tensor([0, 1, npix - 2, npix - 1], device=dev)
    sub = x64[:, :, pick].cpu().numpy()
    want = np.abs(np.fft.fftshift(np.fft.fft(sub, axis=1), axes=1)) ** 2
    got = dst[:, :, pick].cpu().numpy().astype(np.float64)
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert err.max() < 5e-5, (T, err.max())


@pytest.mark.parametrize("T,npix", [(100, 10_700_001), (375, 8_259_001), (500, 2_855_001), (500, 2_857_000), (500, 8_259_001),
                                    (256, 2048 * 2048), (1000, 2_855_001), (1000, 2_857_000)])
def test_tacaw_row_offsets_near_the_32_bit_limit(ps, T, npix):
    """The mixed-radix time kernels address a row as descriptor base + 32-bit offsets; msl_tacaw hands them only images whose
    offsets fit and everything else to the kernels with 64-bit addressing (the buffer unit adds lane offset and scalar offset in
    32 bits: the first version of this test caught the sum wrapping).  One probe, pixel counts just below each limit
    ((T + 1) / 2 rows for the per-lane kernel, 65 rows for one block per wave, TP + (TP + 1) / 2 rows for two blocks per wave) and
    just above (T = 500: the one-block shape of the same L, again up to its own limit, as at 256 frames of a 2048^2 grid; T = 1000:
    the generic LDS kernel): 3 000 random pixels -- the last ones of the image among them, where an overflow would wrap -- against
    the float64 transform, and every element written."""
    import torch
    from pyslice_amd import _native
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T + npix)
    src = torch.randn((1, T, npix, 2), generator=g, device=dev) * 1e-2
    src = torch.view_as_complex(src)
    dst = torch.full((1, T, npix), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng = _native.Engine(2, 2, 1, 1.0, 1.0, 1.0, 1.0, 0.0, n_probes=1, n_frames=0, device=0)
    eng.tacaw(src.data_ptr(), dst.data_ptr(), 1, T, npix)
    eng.synchronize()
    eng.close()
    assert float(dst.min()) >= 0.0
    pick = torch.from_numpy(np.random.default_rng(T).choice(npix, 3000, replace=False)).to(dev)
    pick[:6] = torch.tensor([0, 1, 31, npix - 33, npix - 2, npix - 1], device=dev)
    sub = src[:, :, pick].to(torch.complex128).cpu().numpy()
    sub = sub - sub.mean(axis=1, keepdims=True)
    want = np.abs(np.fft.fftshift(np.fft.fft(sub, axis=1), axes=1)) ** 2
    got = dst[:, :, pick].cpu().numpy().astype(np.float64)
    del src, dst
    torch.cuda.empty_cache()
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    assert err.max() < 5e-5, (T, npix, err.max())


TDIR_LENGTHS = [16, 18, 20, 24, 25, 27, 30, 32, 36, 40, 45, 48, 50, 54, 60, 64, 72, 75, 80, 81, 90, 96, 100, 108, 120, 125, 128,
                21, 28, 35, 42, 49, 56, 63, 70, 84, 98, 105, 112, 126]        # (second line: with a factor 7)
TSPLIT2_LENGTHS = [540, 576, 600, 640, 648, 720, 750, 768, 800, 864, 960, 1000, 1024]       # two blocks per wave
TSPLIT_LENGTHS = [135, 144, 150, 160, 162, 180, 192, 200, 216, 225, 240, 243, 250, 256, 270, 288, 300, 320, 324, 360, 375, 384, 400, 405,
                  432, 450, 480, 486, 500, 512]


@pytest.mark.parametrize("shape", [(7, 9), (20, 30)])
def test_tacaw_smooth_frame_counts_on_the_per_lane_kernel(ps, shape):
    """time_direct_kernel: every 2-3-5-7-smooth frame count from 16 to 128 (radix-4 / 2 / 5 / 3 / 7 register network, one lane per pixel;
    100 = 4.5.5 is the reference notebook's run, example.ipynb:578), and time_split_kernel: every smooth count from 129 to 512 as
    L x TP over the L = 2 .. 6 waves of a workgroup (256 = 2 x 128, 500 = 4 x 125, 486 = 6 x 81 ...) and thirteen counts up to 1024
    as 8 x TP / 6 x TP with two blocks per wave (1000 = 8 x 125).  63 pixels (one ragged tile) and 600 (ragged last tile; with 3 probes more tiles than one per
    workgroup only in the split kernel: 30, the bench covers the rest).  Against the float64 transform per pixel -- strong-mean
    pixels included -- and, bin for bin, against the chirp-z kernel."""
    from pyslice_amd import _native
    nx, ny = shape
    for T in TDIR_LENGTHS + TSPLIT_LENGTHS + TSPLIT2_LENGTHS:
        rng = np.random.default_rng(1000 + T)
        eng = _native.Engine(nx, ny, 1, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=3, n_frames=T)
        big = (rng.standard_normal((3, 1, nx, ny)) + 1j * rng.standard_normal((3, 1, nx, ny))) * 1e2
        big[:, :, ::2, ::3] = 0.0
        small = (rng.standard_normal((3, T, nx, ny)) + 1j * rng.standard_normal((3, T, nx, ny))) * 1e-2
        frames = (big + small).astype(np.complex64)
        f64 = frames.astype(np.complex128)
        want = np.abs(np.fft.fftshift(np.fft.fft(f64 - f64.mean(axis=1, keepdims=True), axis=1), axes=1)) ** 2
        for t in range(T):
            eng.upload_frame(t, frames[:, t])
        eng.tacaw()
        got = eng.intensity().astype(np.float64)
        assert got[:, T // 2].max() == 0.0
        err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
        assert err.max() < 2e-5, (T, err.max())
        os.environ["MSL_DEBUG"] = os.environ["MSL_TACAW_CHIRPZ"] = "1"          # (above 512 frames: the generic LDS kernel)
        try:
            eng.tacaw()
            cz = eng.intensity().astype(np.float64)
        finally:
            del os.environ["MSL_TACAW_CHIRPZ"], os.environ["MSL_DEBUG"]
        eng.close()
        assert not np.array_equal(cz, got), T                     # (two different kernels did run)
        assert rel_l2(got, cz) < 2e-5, T


def test_result_download_as_complex128(ps):
    """msl_download_wavefunction_c128: the (P, T, nx, ny) result in the reference's dtype, widened on the device -- equal, bit for
    bit, to the complex64 download cast on the host; a prefix of the frame slots; several chunks per probe (debug chunk size)."""
    from pyslice_amd import _native
    rng = np.random.default_rng(11)
    eng = _native.Engine(12, 10, 1, 0.1, 0.1, 0.5, 0.037, 1e-3, n_probes=3, n_frames=5)
    frames = (rng.standard_normal((3, 5, 12, 10)) + 1j * rng.standard_normal((3, 5, 12, 10))).astype(np.complex64)
    for t in range(5):
        eng.upload_frame(t, frames[:, t])
    full = eng.wavefunction_c128()
    assert full.dtype == np.complex128 and np.array_equal(full, frames.astype(np.complex128))
    os.environ["MSL_DEBUG"] = "1"
    os.environ["MSL_C128_CHUNK"] = "77"
    try:
        part = eng.wavefunction_c128(4)
    finally:
        del os.environ["MSL_C128_CHUNK"], os.environ["MSL_DEBUG"]
    assert part.shape == (3, 4, 12, 10) and np.array_equal(part, frames[:, :4].astype(np.complex128))
    with pytest.raises(ValueError):                       # (MSL_ERR_INVALID: more frames than slots)
        eng.wavefunction_c128(6)
    eng.close()


def test_result_release_returns_the_device_memory(ps, orc):
    """A WFData from run() keeps the engine (and every device buffer of the run) alive so that TACAWData can work on the resident
    spectra; release() drops that hold: the device memory comes back while the host arrays stay usable -- TACAWData then stages
    the host copy -- and a second setup() on the same calculator does not pile a second set of buffers on top."""
    import gc
    import torch
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(256, 4, 6, density=0.03, seed=2)
    pp = [(5.0, 5.0), (12.0, 20.0), (3.0, 17.0), (21.0, 9.0)]
    gc.collect()
    free0, _ = torch.cuda.mem_get_info(0)
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)          # the first run's engine now lives in `wf` only
    free_two, _ = torch.cuda.mem_get_info(0)
    wf.release()
    gc.collect()
    free_one, _ = torch.cuda.mem_get_info(0)
    assert free_one - free_two > 4 * 6 * 256 * 256 * 8                            # at least the (P,T,nx,ny) spectra came back
    assert rel_l2(npy(wf.wavefunction_data), want) < WAVE_TOL
    f, inten = orc.tacaw(want, wf.time)
    assert rel_l2(npy(ps.TACAWData(wf).intensity), inten) < TACAW_TOL             # staged from the host arrays
    del calc
    gc.collect()
    torch.cuda.empty_cache()
    assert free0 - torch.cuda.mem_get_info(0)[0] < 512 << 20        # (code objects, the staged copy `wf` still holds, allocator slack)


def test_handle_teardown_returns_all_device_memory(ps):
    """Create, use and destroy a handle three times in one process: a thickness series (msl_set_layers), a TACAW call of every
    kind of time kernel (four-step, per-lane, wave-split, chirp-z, generic: each with tables of its own in the handle), the
    resident and the layer TACAW, a stream begin / push / finish, detectors and a diffraction call.  Every device buffer of the
    handle must come back with msl_destroy: the free device memory after the third cycle is within ONE per-probe work buffer of
    this configuration (1024 x 1024 x 16 probes x 8 bytes = 128 MB without its row padding, far above allocator granularity) of
    the value after the first.  Only normal teardown is watched: nothing here fails an allocation."""
    import gc
    import torch
    from pyslice_amd import _native
    from pyslice_amd.synthetic import synthetic_trajectory
    from pyslice_amd.potentials import slice_edges
    n, nz, P, T = 1024, 2, 16, 2
    dev = torch.device("cuda", 0)
    tr = synthetic_trajectory(n, nz, 1, density=0.02, seed=3)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    pp = np.random.default_rng(2).random((P, 2)) * [lx, ly]
    kirkland = ps.loadKirkland()
    # the caller's TACAW buffers live through all cycles (torch's caching allocator stays out of the comparison)
    npix = 4096
    time_cases = [(100, {}), (256, {}), (1024, {"MSL_TACAW_FOURSTEP": "1"}), (97, {}), (1030, {})]   # direct, split, four-step, chirp-z, generic
    src = torch.view_as_complex(torch.randn((1, 1030, npix, 2), device=dev))
    dst = torch.empty((1, 1030, npix), dtype=torch.float32, device=dev)
    k = np.fft.fftshift(np.fft.fftfreq(n, 0.1)).astype(np.float32)
    member = np.ones(n * n, dtype=np.uint16)
    torch.cuda.synchronize()

    def cycle():
        eng = _native.Engine(n, n, nz, xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], 0.0370144, 9.24396e-4, n_probes=P, n_frames=T)
        eng.set_kirkland(kirkland)
        eng.set_slices(*slice_edges(zs))
        eng.set_probes(30.0, pp)
        eng.set_layers([0])
        eng.build_potential(tr.positions[0], tr.atom_types.astype(np.int32))
        for t in range(T):
            eng.propagate_frame(t)
        eng.tacaw()
        eng.tacaw_layer(0)
        for frames, switches in time_cases:
            env = dict(switches, MSL_DEBUG="1") if switches else {}
            os.environ.update(env)
            try:
                eng.tacaw(src.data_ptr(), dst.data_ptr(), 1, frames, npix)
            finally:
                for name in env:
                    del os.environ[name]
        eng.tacaw_stream_begin(T)
        eng.tacaw_stream_push(0, T, 0)
        assert eng.tacaw_stream_finish().shape == (P, n, n)
        eng.set_detectors(member, ["intensity"], k, k)
        assert eng.detect().shape == (P, T, 1)
        assert eng.diffract(bin=(4, 4)).shape == (P, n // 4, n // 4)
        eng.synchronize()
        eng.close()
        gc.collect()
        return torch.cuda.mem_get_info(0)[0]

    free = [cycle() for _ in range(3)]
    print(f"free device memory after each cycle: {free}, third - first = {free[2] - free[0]} bytes")
    assert abs(free[2] - free[0]) < n * n * P * 8, free


def test_tacaw_time_axis_256_frames(ps, orc):
    """T = 256 frames (BASELINE C3's frame count) through the calculator: the wave-split register kernel (2 x 128; the
    four-step column kernel until round 3), DC zeroed, fftshifted |.|^2; compare with the oracle and with the generic kernel."""
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(32, 2, 256, density=0.3, seed=13)
    pp = [(1.6, 1.6), (0.5, 2.5)]
    calc = ps.MultisliceCalculator(progress=False)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    data = npy(wf.wavefunction_data)
    tac = ps.TACAWData(wf)
    f, inten = orc.tacaw(data, wf.time)
    got = npy(tac.intensity)
    assert got.shape == (2, 256, 32, 32)
    assert np.allclose(tac.frequencies, f)
    assert rel_l2(got, inten) < TACAW_TOL
    assert got[:, 128].max() == 0.0
    os.environ["MSL_DEBUG"] = os.environ["MSL_TACAW_GENERIC"] = "1"
    try:
        calc._engine.tacaw()
        gen = calc._engine.intensity()
    finally:
        del os.environ["MSL_TACAW_GENERIC"], os.environ["MSL_DEBUG"]
    assert rel_l2(got, gen) < 1e-5


@pytest.mark.parametrize("nx,ny,T,P,window", [(45, 37, 20, 3, None), (64, 64, 12, 2, (21, 19)), (33, 31, 100, 2, None)])
def test_results_on_odd_pixel_counts_sit_at_a_line_aligned_pitch(ps, orc, nx, ny, T, P, window):
    """Library-owned (P,T,wx,wy) results keep every image at msl_result_pitch() pixels (a multiple of 32), so that the time
    kernels move whole lines on grids like the reference's 501 x 491 (00_probe.py:7-8; tacaw_data.py:94-104 runs over exactly
    such arrays).  Everything that hides or carries the pitch, against the oracle: dense downloads (complex64, complex128, one
    frame), the strided zero-copy views (output='device'), the time FFT, every reduction from the library's own buffer and
    through a pointer into it, ADF, and the frame up/download used by the cache."""
    import torch
    from pyslice_amd import _native
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, 3, T, ny=ny, density=0.08, seed=5 + T)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(3).random((P, 2)) * [lx, ly]]
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    if window:
        x0, y0 = nx // 2 - window[0] // 2, ny // 2 - window[1] // 2
        want = want[:, :, x0:x0 + window[0], y0:y0 + window[1]]
    wx, wy = want.shape[2], want.shape[3]
    f, inten = orc.tacaw(want, np.arange(T) * tr.timestep)
    calc = ps.MultisliceCalculator(progress=False, output="device", k_window=window)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    wf = calc.run()
    eng = calc._engine
    pitch = eng.result_pitch(_native.BUF_WAVEFUNCTION)
    assert pitch % 32 == 0 and wx * wy <= pitch < wx * wy + 32 and (wx * wy) % 32 != 0
    assert eng.buffer_bytes(_native.BUF_WAVEFUNCTION) == P * T * pitch * 8
    view = wf.wavefunction_data                                     # strided zero-copy view, (P, T, wx, wy, 1)
    assert tuple(view.shape) == (P, T, wx, wy, 1) and view.stride()[1] == pitch and not view.is_contiguous()
    assert rel_l2(npy(view), want) < 1e-4
    host = eng.wavefunction()
    assert np.array_equal(host, npy(view)[..., 0])
    assert np.array_equal(eng.wavefunction(first=1, count=P - 1), host[1:])
    assert np.array_equal(eng.wavefunction_c128(T - 1), host[:, :T - 1].astype(np.complex128))
    assert np.array_equal(eng.frame(T // 2), host[:, T // 2])
    # pad pixels hold zeros, before and after the time FFT
    raw = torch.as_tensor(_native.DeviceArray(eng.device_ptr(_native.BUF_WAVEFUNCTION), (P, T, pitch), "<c8", owner=eng), device="cuda")
    assert float(raw[:, :, wx * wy:].abs().max()) == 0.0
    tac = ps.TACAWData(wf)
    got = npy(tac.intensity)
    assert got.shape == inten.shape and rel_l2(got, inten) < TACAW_TOL
    assert eng.result_pitch(_native.BUF_INTENSITY) == pitch and not tac.intensity.is_contiguous()
    assert np.array_equal(eng.intensity(), got.astype(np.float32))
    assert np.array_equal(eng.intensity(first=P - 1, count=1), got[P - 1:].astype(np.float32))
    kxs, kys = npy(wf.kxs), npy(wf.kys)
    mask = np.hypot(kxs[:, None], kys[None, :]) < 0.6 * max(np.abs(kxs).max(), np.abs(kys).max())
    soft = np.exp(-(kxs[:, None] ** 2 + kys[None, :] ** 2) / 3.0)
    I = inten
    assert rel_l2(tac.spectrum(None), I.sum(axis=(2, 3)).mean(axis=0)) < TACAW_TOL
    assert rel_l2(tac.spectrum(P - 1), I[P - 1].sum(axis=(1, 2))) < TACAW_TOL
    assert rel_l2(tac.diffraction(None), I.sum(axis=1).mean(axis=0)) < TACAW_TOL
    assert rel_l2(tac.diffraction(1), I[1].sum(axis=0)) < TACAW_TOL
    fq = float(f[T // 2 + 2])
    assert rel_l2(tac.spectral_diffraction(fq, 0), I[0, T // 2 + 2]) < TACAW_TOL
    assert rel_l2(tac.spectrum_image(fq), I[:, T // 2 + 2].sum(axis=(1, 2))) < TACAW_TOL
    assert rel_l2(tac.masked_spectrum(mask, 1), (I[1] * mask[None]).sum(axis=(1, 2))) < TACAW_TOL
    assert rel_l2(tac.masked_spectrum(mask), (I * mask[None, None]).sum(axis=(2, 3)).mean(axis=0)) < TACAW_TOL
    assert rel_l2(tac.masked_spectrum(soft, P - 1), (I[P - 1] * soft[None]).sum(axis=(1, 2))) < TACAW_TOL
    ix, iy = [0, wx // 2, wx - 1], [wy - 1, wy // 3, 0]
    assert rel_l2(tac.dispersion(kxs[ix], kys[iy], 1), I[1][:, ix, iy]) < TACAW_TOL
    # ADF over the resident exit waves (haadf_data.py:72-94) with the last pixel of an image inside the mask
    m = np.ones((wx, wy), dtype=bool); m[: wx // 2] = False
    assert rel_l2(eng.adf(m), (np.abs(want[..., 0]) * m).sum(axis=(2, 3)).mean(axis=1)) < 1e-4
    # the cache path: a frame written back lands where it came from
    frame = (host[:, 3] * 2).astype(np.complex64)
    eng.upload_frame(3, frame)
    assert np.array_equal(eng.frame(3), frame) and np.array_equal(eng.frame(2), host[:, 2]) and np.array_equal(eng.frame(4), host[:, 4])
    assert float(raw[:, :, wx * wy:].abs().max()) == 0.0


def test_streaming_tacaw_on_an_odd_pixel_window(ps, orc):
    """The frame ring of a streaming run keeps its images at the line-aligned pixel pitch too (21 x 19 = 399 pixels at 416): the fold
    reads the ring with that pitch, the reference pattern is copied out of it row by row, the accumulators and the finished
    intensity are dense (tacaw_data.py:89-104 on a k-window)."""
    from pyslice_amd import _native
    from pyslice_amd.synthetic import synthetic_trajectory
    n, T, P, win, tile = 64, 10, 2, (21, 19), 4
    tr = synthetic_trajectory(n, 3, T, density=0.08, seed=77)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(8).random((P, 2)) * [lx, ly]]
    full = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    x0, y0 = n // 2 - win[0] // 2, n // 2 - win[1] // 2
    f, inten = orc.tacaw(full[:, :, x0:x0 + win[0], y0:y0 + win[1]], np.arange(T) * tr.timestep)
    calc = ps.MultisliceCalculator(progress=False, stream_tile=tile, k_window=win)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert calc._engine.result_pitch(_native.BUF_WAVEFUNCTION) == 416
    tac = calc.run_streaming_tacaw()
    got = npy(tac.intensity)
    assert got.shape == inten.shape and rel_l2(got, inten) < TACAW_TOL
    assert rel_l2(tac.total_diffraction, inten.sum(axis=1)) < TACAW_TOL
    assert rel_l2(tac.spectrum(1), inten[1].sum(axis=(1, 2))) < TACAW_TOL
    assert rel_l2(tac.diffraction(0), inten[0].sum(axis=0)) < TACAW_TOL
