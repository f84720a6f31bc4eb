"""Frozen phonons on the MI355X: the positions the device generates against the NumPy definition (thermal.py), the potential
build behind them against msl_build_potentials fed the same positions (bit for bit), random access by configuration index, the
calculator's run modes against the same modes on the materialised trajectory, and the teardown of the resident structure.

Cells: 1061 atoms of three species, uniformly random in the box with 1 A of vacuum below and above along the slice axis (the
largest displacement there is, 0.12 A x 6.77, stays inside), per-atom widths in [0, 0.12] A with exact zeros; 0.1 A pixels, 1 A
slices, 100 kV.  128 x 96 x 4 runs on the convolution kernels, 256 x 256 x 3 on the four-step kernels."""
import functools

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

EV = 100e3
N_ATOMS = 1061
SHAPES = [(128, 96, 4), (256, 256, 3)]
SEEDS = [0, 2 ** 32 + 3]
CONFIGS = [0, 7, 2 ** 32 + 5]
PP = [(3.05, 4.4), (7.7, 1.25), (0.0, 0.0), (11.3, 8.05)]


def npy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


@functools.lru_cache(maxsize=None)
def phonons(nx, ny, nz, n_configs=5, seed=SEEDS[1]):
    """the FrozenPhonons of a grid (read-only arrays: shared by the tests)"""
    from pyslice_amd.synthetic import box_for_grid
    from pyslice_amd.thermal import FrozenPhonons
    box = box_for_grid(nx, nz, 0.1, 1.0, ny)
    rng = np.random.default_rng(nx + ny + nz)
    lo, span = np.array([0.0, 0.0, 1.0]), np.array([box[0, 0], box[1, 1], box[2, 2] - 2.0])
    assert span[2] > 0
    pos = lo + rng.random((N_ATOMS, 3)) * span
    Z = np.array([38, 22, 8])[rng.integers(0, 3, N_ATOMS)]
    sigma = rng.random(N_ATOMS) * 0.12
    sigma[rng.random(N_ATOMS) < 0.1] = 0.0
    sigma[:3] = [0.0, 0.12, 0.0]
    fp = FrozenPhonons(Z, pos, box, sigma, n_configs, seed=seed)
    for a in (fp.positions, fp.sigma, fp.atom_types):
        a.setflags(write=False)
    return fp


@functools.lru_cache(maxsize=None)
def materialised(nx, ny, nz):
    """the definition's configurations as a Trajectory, computed once"""
    tr = phonons(nx, ny, nz).to_trajectory()
    tr.positions.setflags(write=False)
    return tr


def make_engine(ps, fp, P=2, n_frames=4, frame_batch=4, slice_axis=2, structure=True):
    """an engine on the grid of fp with its probes set; slice_axis = 0 reads the slice coordinate from column 0 and the in-plane
    coordinates from columns 1, 2 (pos_for_axis permutes the columns to match)"""
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import slice_edges
    xs, ys, zs = ps.gridFromTrajectory(fp, 0.1, 1.0)[:3]
    eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(EV), interaction_sigma(EV),
                         n_probes=P, n_frames=n_frames, frame_batch=frame_batch)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(zs))
    eng.set_probes(30.0, np.asarray(PP[:P]))
    if structure:
        eng.set_structure(pos_for_axis(fp.positions, slice_axis), fp.atom_types, fp.sigma, slice_axis)
    return eng


def pos_for_axis(pos, slice_axis):
    return np.ascontiguousarray(pos if slice_axis == 2 else pos[..., [2, 0, 1]])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ---- the positions -----------------------------------------------------------------------------------------
def test_device_positions_match_the_definition(ps):
    """max |delta| <= 1e-12 A: the device's double log / sqrt / sincospi are good to a few ulp (displacement error below 1e-15), the
    final sum rounds to half an ulp of a coordinate below 1e3 A, 1.1e-13: a tenfold margin.  sigma = 0 atoms: the base, bit for bit."""
    from pyslice_amd import thermal
    fp = phonons(*SHAPES[0])
    eng = make_engine(ps, fp)
    still = fp.sigma == 0
    assert 50 < still.sum() < 300 and fp.sigma.max() == 0.12 and len(set(fp.atom_types.tolist())) == 3
    try:
        for seed in SEEDS:
            for config in CONFIGS:
                got = eng.thermal_positions(seed, config)
                want = thermal.displaced(fp.positions, fp.sigma, seed, config)
                err = np.abs(got - want).max()
                print(f"seed {seed} config {config}: max |device - definition| = {err:.3e} A")
                assert got.shape == (N_ATOMS, 3) and err <= 1e-12
                assert np.array_equal(bits(got[still]), bits(fp.positions[still]))
                assert (got[~still] != fp.positions[~still]).all()
        assert not np.array_equal(eng.thermal_positions(0, 5), eng.thermal_positions(0, 2 ** 32 + 5))
        assert not np.array_equal(eng.thermal_positions(3, 5), eng.thermal_positions(2 ** 32 + 3, 5))
    finally:
        eng.close()


def test_refusals(ps):
    fp = phonons(*SHAPES[0])
    eng = make_engine(ps, fp, structure=False)
    try:
        with pytest.raises(ValueError, match="msl_set_structure"):
            eng.build_thermal(0, 0, 1)
        with pytest.raises(ValueError, match="msl_set_structure"):
            eng.thermal_positions(0, 0)
        bad = fp.sigma.copy()
        bad[17] = -0.01
        with pytest.raises(ValueError, match="width"):
            eng.set_structure(fp.positions, fp.atom_types, bad)
        bad[17] = np.nan
        with pytest.raises(ValueError, match="width"):
            eng.set_structure(fp.positions, fp.atom_types, bad)
        Z = fp.atom_types.copy()
        Z[5] = 104
        with pytest.raises(ValueError, match="atomic number 104"):
            eng.set_structure(fp.positions, Z, fp.sigma)
        with pytest.raises(ValueError, match="msl_set_structure"):             # a refused structure is no structure
            eng.build_thermal(0, 0, 1)
        eng.set_structure(fp.positions, fp.atom_types, fp.sigma)
        for first, count in ((0, 0), (0, 5), (-1, 1)):
            with pytest.raises(ValueError):
                eng.build_thermal(0, first, count)
        eng.build_thermal(0, 0, 4)
        eng.synchronize()
    finally:
        eng.close()


# ---- the same pipeline behind the positions ----------------------------------------------------------------
@pytest.mark.parametrize("slice_axis", [2, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_build_thermal_is_build_potentials_of_the_same_positions(ps, shape, slice_axis):
    """A: build_thermal + propagate_frames.  B (another handle): build_potentials of the stacked thermal_positions + propagate_frames.
    Everything behind d_pos is the same deterministic kernels: the exit spectra are equal bit for bit.  count = 3 at frame_batch = 4,
    then count = 1 at frame_batch = 1."""
    fp = phonons(*shape)
    seed = fp.seed
    for fb, count in ((4, 3), (1, 1)):
        A = make_engine(ps, fp, frame_batch=fb, slice_axis=slice_axis)
        B = make_engine(ps, fp, frame_batch=fb, slice_axis=slice_axis, structure=False)
        try:
            pos = np.stack([A.thermal_positions(seed, 3 + k) for k in range(count)])
            Z = np.asarray(fp.atom_types, dtype=np.int32)
            if fb > 1:
                A.build_thermal(seed, 3, count)
                A.propagate_frames(0, count)
                B.build_potentials(pos, Z, slice_axis)
                B.propagate_frames(0, count)
            else:
                A.build_thermal(seed, 3, 1)
                A.propagate_frame(0)
                B.build_potential(pos[0], Z, slice_axis)
                B.propagate_frame(0)
            a, b = A.wavefunction()[:, :count], B.wavefunction()[:, :count]
            assert np.isfinite(a).all() and np.abs(a).max() > 0
            assert np.array_equal(bits(a), bits(b)), (fb, count, rel_l2(a, b))
            assert np.array_equal(bits(A.transmission()), bits(B.transmission()))
            if count > 1:                                           # the configurations differ from one another
                assert not np.array_equal(a[:, 0], a[:, 1])
        finally:
            A.close()
            B.close()


def test_slice_axis_does_not_change_the_configuration(ps):
    """g_x, g_y, g_z belong to the columns of the positions array, not to the in-plane and slice axes: the displacements of a
    structure at the origin, whichever axis is the slice axis"""
    fp = phonons(*SHAPES[0])
    A = make_engine(ps, fp, structure=False)
    B = make_engine(ps, fp, structure=False)
    try:
        A.set_structure(np.zeros((N_ATOMS, 3)), fp.atom_types, fp.sigma, 2)
        B.set_structure(np.zeros((N_ATOMS, 3)), fp.atom_types, fp.sigma, 0)
        a, b = A.thermal_positions(9, 4), B.thermal_positions(9, 4)
        assert np.abs(a).max() > 0.1 and np.array_equal(bits(a), bits(b))
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_random_access(ps, shape):
    """configuration 5 after configurations 0..2 is configuration 5 of a fresh handle, and the same again when asked twice"""
    fp = phonons(*shape)
    seed = fp.seed
    A = make_engine(ps, fp)
    B = make_engine(ps, fp)
    try:
        A.build_thermal(seed, 0, 3)
        A.propagate_frames(0, 3)
        first = A.wavefunction()[:, :3]
        A.build_thermal(seed, 5, 1)
        A.propagate_frames(0, 1)
        a = A.wavefunction()[:, 0]
        A.build_thermal(seed, 5, 1)
        A.propagate_frames(1, 1)
        again = A.wavefunction()[:, 1]
        B.build_thermal(seed, 5, 1)
        B.propagate_frames(0, 1)
        b = B.wavefunction()[:, 0]
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(again))
        assert not np.array_equal(a, first[:, 0])
        # ... and a Trajectory-style build on the same handle in between leaves the structure as it is
        A.build_potentials(np.zeros((2, 1, 3)) + 1.2, np.array([79], dtype=np.int32))
        A.build_thermal(seed, 5, 1)
        A.propagate_frames(2, 1)
        assert np.array_equal(bits(A.wavefunction()[:, 2]), bits(b))
    finally:
        A.close()
        B.close()


# ---- the calculator ----------------------------------------------------------------------------------------
def _no_atom_near_a_slice_edge(ps, fp, tr):
    """on the CPU: no atom of any definition configuration within 1e-9 A of a slice edge, so that the 1e-13 A between the device's
    positions and the definition's cannot move an atom to another slice"""
    from pyslice_amd.potentials import slice_edges
    zs = ps.gridFromTrajectory(fp, 0.1, 1.0)[2]
    lo, hi = slice_edges(zs)
    edges = np.unique(np.concatenate([lo, hi]))
    z = tr.positions[..., 2]
    assert z.min() > lo[0] + 1e-9 and z.max() < hi[-1] - 1e-9
    assert np.abs(z[..., None] - edges).min() > 1e-9


@pytest.mark.parametrize("shape", SHAPES)
def test_run_matches_the_definition(ps, shape):
    """MultisliceCalculator.run() on the FrozenPhonons against run() on its to_trajectory(): 5 configurations, 2 probes, rel-L2 <=
    1e-4 on the wavefunctions (the parity contract)"""
    fp, tr = phonons(*shape), materialised(*shape)
    _no_atom_near_a_slice_edge(ps, fp, tr)
    out = []
    for source in (fp, tr):
        calc = ps.MultisliceCalculator(progress=False, frame_batch=2, dtype="complex64")
        calc.setup(source, aperture=30.0, voltage_eV=EV, slice_thickness=1.0, probe_positions=PP[:2])
        assert (calc.nx, calc.ny, calc.nz) == shape
        wf = calc.run()
        out.append(npy(wf.wavefunction_data))
        assert np.allclose(wf.time, np.arange(5) * fp.timestep)
    assert out[0].shape == (2, 5) + shape[:2] + (1,)
    err = rel_l2(out[0], out[1])
    print(f"{shape}: run() on FrozenPhonons against its to_trajectory(): rel-L2 {err:.3e}")
    assert err <= 1e-4
    assert rel_l2(out[1][:, 0], out[1][:, 1]) > 1e-3               # (the configurations are not one another)


def _mode_runs(ps, shape, run, **kw):
    fp, tr = phonons(*shape), materialised(*shape)
    _no_atom_near_a_slice_edge(ps, fp, tr)
    out = []
    for source in (fp, tr):
        calc = ps.MultisliceCalculator(progress=False, frame_batch=2, probe_batch=2, **kw)
        calc.setup(source, aperture=30.0, voltage_eV=EV, slice_thickness=1.0, probe_positions=PP)
        out.append(getattr(calc, run)())
    return out


def _stem_agree(ps, got, want):
    """the bounds test_gpu_detectors.py holds run_detectors() to against its host comparison"""
    kmax = max(np.abs(npy(got.kxs)).max(), np.abs(npy(got.kys)).max())
    assert got.signals.shape == want.signals.shape == (4, 5, 2)
    total = want.signals[..., 0].max()                          # (the bright-field disc: no more than the whole pattern they scale by)
    for d, det in enumerate(got.detectors):
        if det.signal.startswith("com"):
            err = np.abs(got.signals[..., d] - want.signals[..., d]).max()
            print(f"{det.name}: max |diff| {err:.3e} (bound {1e-4 * kmax * total:.3e})")
            assert err <= 1e-4 * kmax * total, det.name
        else:
            err = rel_l2(got.signals[..., d], want.signals[..., d])
            print(f"{det.name}: rel-L2 {err:.3e}")
            assert err <= 1e-4, det.name


def _detectors(ps):
    return [ps.Detector("bf", outer=30.0), ps.Detector("comx", outer=60.0, signal="com_x")]


def test_run_detectors_matches_the_definition(ps):
    got, want = _mode_runs(ps, SHAPES[0], "run_detectors", detectors=_detectors(ps))
    _stem_agree(ps, got, want)


def test_run_diffraction_split_matches_the_definition(ps):
    """probe batches outside, frames inside: every probe batch regenerates the five configurations by index"""
    got, want = _mode_runs(ps, SHAPES[0], "run_diffraction", diffraction=ps.Diffraction(bin=(4, 4), split=True))
    assert got.intensity.shape == want.intensity.shape == (4, 32, 24)
    for name in ("intensity", "elastic"):
        errs = [rel_l2(getattr(got, name)[p], getattr(want, name)[p]) for p in range(4)]
        print(f"{name}: max rel-L2 per pattern {max(errs):.3e}")
        assert max(errs) <= 2e-4, name
    assert (want.elastic < want.intensity).any()


def test_prism_detectors_match_the_definition(ps):
    from pyslice_amd.prism import Prism
    got, want = _mode_runs(ps, SHAPES[0], "run_detectors", detectors=_detectors(ps), prism=Prism(1))
    _stem_agree(ps, got, want)


# ---- teardown ----------------------------------------------------------------------------------------------
def test_structure_teardown_returns_all_device_memory(ps):
    """set_structure / build_thermal / thermal_positions / destroy, three times in one process (the pattern of
    test_handle_teardown_returns_all_device_memory): free device memory after the third cycle is within the smallest resident
    buffer of the structure (Z of 2^21 atoms: 8 MiB; the widths are 16 MiB, the positions 48) of the value after the first."""
    import gc
    import torch
    from pyslice_amd.thermal import FrozenPhonons
    from pyslice_amd.synthetic import box_for_grid
    n = 1 << 21
    rng = np.random.default_rng(1)
    box = box_for_grid(64, 2, 0.1, 1.0)
    fp = FrozenPhonons(np.array([14, 8])[rng.integers(0, 2, n)], rng.random((n, 3)) * np.diag(box), box, 0.05, 2)
    torch.cuda.synchronize()

    def cycle():
        eng = make_engine(ps, fp, P=1, n_frames=2, frame_batch=2, structure=False)
        eng.set_structure(fp.positions, fp.atom_types, fp.sigma)
        eng.set_structure(fp.positions, fp.atom_types, fp.sigma)         # (a second structure replaces the first)
        eng.build_thermal(1, 0, 2)
        eng.propagate_frames(0, 2)
        assert eng.thermal_positions(1, 1).shape == (n, 3)
        eng.synchronize()
        eng.close()
        gc.collect()
        return torch.cuda.mem_get_info(0)[0]

    free = [cycle() for _ in range(3)]
    print(f"free device memory after each cycle: {free}, third - first = {free[2] - free[0]} bytes")
    assert abs(free[2] - free[0]) < n * 4, free
