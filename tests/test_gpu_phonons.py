"""Phonon modes on the MI355X: the positions the device synthesises against the NumPy definition (phonons.py), the potential build
behind them against msl_build_potentials fed the same positions (bit for bit), random access by frame index, the calculator's run
modes against the same modes on the materialised trajectory, the refusals and the teardown of the resident modes.

Cells as in test_gpu_thermal.py: atoms uniformly random in the box with 1 A of vacuum below and above along the slice axis, 0.1 A
pixels, 1 A slices, 100 kV; 128 x 96 x 4 runs on the convolution kernels, 256 x 256 x 3 on the four-step kernels.  Modes: wave
vectors up to 2 cycles / A (not commensurate with the box), phase advances in [0, 1), complex displacement vectors of
0.03 / sqrt(M) A so that the displacements stay near 0.03 A whatever M is."""
import functools

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

EV = 100e3
EPS = 2.0 ** -52
N_ATOMS = 1061
SHAPES = [(128, 96, 4), (256, 256, 3)]
SEEDS = [0, 2 ** 32 + 3]
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
def modes(nx, ny, nz, n_atoms=N_ATOMS, M=37, nb=3, dynamic=True, n_frames=5, seed=SEEDS[1], still=True):
    """the PhononModes of a grid (read-only arrays: shared by the tests); with `still` and nb > 1 basis atom 1 does not move"""
    from pyslice_amd.synthetic import box_for_grid
    from pyslice_amd.phonons import PhononModes
    box = box_for_grid(nx, nz, 0.1, 1.0, ny)
    rng = np.random.default_rng(nx + ny + nz + 7 * n_atoms + 11 * M + 13 * nb)
    lo, span = np.array([0.0, 0.0, 1.0]), np.array([box[0, 0], box[1, 1], box[2, 2] - 2.0])
    assert span[2] > 0
    pos = lo + rng.random((n_atoms, 3)) * span
    Z = np.array([38, 22, 8])[rng.integers(0, 3, n_atoms)]
    b = rng.integers(0, nb, n_atoms)
    b[:min(nb, n_atoms)] = np.arange(min(nb, n_atoms))
    q = (rng.random((M, 3)) - 0.5) * 4.0
    nu = rng.random(M)
    W = (rng.standard_normal((M, nb, 3)) + 1j * rng.standard_normal((M, nb, 3))) * (0.03 / np.sqrt(M))
    if still and nb > 1:
        W[:, 1, :] = 0.0
    pm = PhononModes(Z, pos, box, b, q, nu, W, n_frames, seed=seed, dynamic=dynamic)
    for a in (pm.positions, pm.atom_types, pm.basis_index, pm.wavevectors, pm.frequencies, pm.tau, pm.displacements):
        a.setflags(write=False)
    return pm


@functools.lru_cache(maxsize=None)
def materialised(nx, ny, nz):
    """the definition's frames as a Trajectory, computed once"""
    tr = modes(nx, ny, nz).to_trajectory()
    tr.positions.setflags(write=False)
    return tr


def pos_for_axis(pos, slice_axis):
    return np.ascontiguousarray(pos if slice_axis == 2 else pos[..., [2, 0, 1]])


def make_engine(ps, pm, P=2, n_frames=4, frame_batch=4, slice_axis=2, structure=True, set_modes=True, dynamic=None):
    """an engine on the grid of pm with its probes set (make_engine of test_gpu_thermal.py, with the modes on top)"""
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import slice_edges
    xs, ys, zs = ps.gridFromTrajectory(pm, 0.1, 1.0)[:3]
    eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(EV), interaction_sigma(EV),
                         n_probes=P, n_frames=n_frames, frame_batch=frame_batch)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(zs))
    eng.set_probes(30.0, np.asarray(PP[:P]))
    if structure:
        eng.set_structure(pos_for_axis(pm.positions, slice_axis), pm.atom_types, np.zeros(pm.n_atoms), slice_axis)
        if set_modes:
            put_modes(eng, pm, dynamic)
    return eng


def put_modes(eng, pm, dynamic=None):
    eng.set_modes(pm.basis_index, pm.wavevectors, pm.tau, pm.displacements, pm.dynamic if dynamic is None else dynamic)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ---- the positions -----------------------------------------------------------------------------------------
POSITION_CASES = [(n, M, nb) for n in (1, 257, 1061) for M in (1, 37, 300) for nb in (1, 3)] + [(257, 37, 40)]


@pytest.mark.parametrize("n_atoms,M,nb", POSITION_CASES)
def test_device_positions_match_the_definition(ps, n_atoms, M, nb):
    """per atom |delta| <= (M + 64) 2^-52 S_i + 2.3e-13 A, S_i = 2 sum_m |g_m| max_alpha |W[m, b_i, alpha]| from the definition's own
    tables: the forward bound of an M-term recursive sum whose terms carry a few roundings each, plus one ulp of a coordinate below
    1e3 A.  M = 1 is a lone mode, 37 a full chunk of 32 and a partial one, 300 nine chunks and a remainder; n_atoms = 1 and 257 leave
    a workgroup nearly empty, 1061 is five workgroups; the one case of nb = 40 reads the W rows from global memory (more than 16
    basis atoms).  The atoms of a basis atom whose W rows are zero come back as the base, bit for bit.  Dynamic records at frames 0 and 7, snapshots at
    0, 7 and 2^32 + 5; seeds 0 and 2^32 + 3."""
    from pyslice_amd import phonons
    pm = modes(*SHAPES[0], n_atoms=n_atoms, M=M, nb=nb)
    eng = make_engine(ps, pm, set_modes=False)
    still = (pm.basis_index == 1) if nb > 1 else np.zeros(n_atoms, dtype=bool)
    Wmax = np.abs(pm.displacements).max(axis=2)                              # (M, nb)
    worst = 0.0
    try:
        for dynamic, frames in ((True, (0, 7)), (False, (0, 7, 2 ** 32 + 5))):
            put_modes(eng, pm, dynamic)
            for seed in SEEDS:
                for frame in frames:
                    got = eng.mode_positions(seed, frame)
                    want = phonons.displaced(pm.positions, pm.basis_index, pm.wavevectors, pm.tau, pm.displacements, seed, frame, dynamic)
                    g = np.abs(phonons.normal_coordinates(seed, 0 if dynamic else frame, M))
                    S = 2.0 * (g[:, None] * Wmax).sum(axis=0)[pm.basis_index]
                    bound = (M + 64) * EPS * S + 2.3e-13
                    err = np.abs(got - want).max(axis=1)
                    worst = max(worst, (err / bound).max())
                    print(f"n {n_atoms} M {M} nb {nb} dynamic {dynamic} seed {seed} frame {frame}: max |device - definition| = "
                          f"{err.max():.3e} A, max over atoms of |delta| / bound = {(err / bound).max():.3f}")
                    assert got.shape == (n_atoms, 3) and (err <= bound).all()
                    assert np.array_equal(bits(got[still]), bits(pm.positions[still]))
                    assert (got[~still] != pm.positions[~still]).any(axis=1).all()
            a, b = eng.mode_positions(3, 5), eng.mode_positions(2 ** 32 + 3, 5)
            assert not np.array_equal(a, b)
        assert not np.array_equal(eng.mode_positions(0, 5), eng.mode_positions(0, 2 ** 32 + 5))       # (snapshots: all 64 bits)
    finally:
        eng.close()
    print(f"worst |delta| / bound: {worst:.3f}")


def test_slice_axis_does_not_change_the_frame(ps):
    """q, W and the displacements belong to the columns of the positions array, not to the in-plane and slice axes"""
    pm = modes(*SHAPES[0])
    A = make_engine(ps, pm, structure=False)
    B = make_engine(ps, pm, structure=False)
    try:
        A.set_structure(pm.positions, pm.atom_types, np.zeros(N_ATOMS), 2)
        B.set_structure(pm.positions, pm.atom_types, np.zeros(N_ATOMS), 0)
        put_modes(A, pm)
        put_modes(B, pm)
        a, b = A.mode_positions(9, 4), B.mode_positions(9, 4)
        assert np.abs(a - pm.positions).max() > 0.01 and np.array_equal(bits(a), bits(b))
    finally:
        A.close()
        B.close()


# ---- the same pipeline behind the positions ----------------------------------------------------------------
@pytest.mark.parametrize("slice_axis", [2, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_build_modes_is_build_potentials_of_the_same_positions(ps, shape, slice_axis):
    """A: build_modes + propagate_frames.  B (another handle): build_potentials of the stacked mode_positions + propagate_frames.
    Everything behind d_pos is the same deterministic kernels: the exit spectra and the transmission functions are equal bit for bit.
    count = 3 at frame_batch = 4 (the tile of 8 frames, partly filled), count = 1 at frame_batch = 1 (the tile of 2), and on the small
    cell count = 2 at frame_batch = 2 (the tile of 2, full) and count = 11 at frame_batch = 11: a full tile of 8 and a partial one."""
    pm = modes(*shape)
    seed = pm.seed
    for fb, count in ((4, 3), (1, 1)) + (((2, 2), (11, 11)) if shape == SHAPES[0] else ()):
        A = make_engine(ps, pm, n_frames=max(4, count), frame_batch=fb, slice_axis=slice_axis)
        B = make_engine(ps, pm, n_frames=max(4, count), frame_batch=fb, slice_axis=slice_axis, structure=False)
        try:
            pos = np.stack([A.mode_positions(seed, 3 + k) for k in range(count)])
            Z = np.asarray(pm.atom_types, dtype=np.int32)
            if fb > 1:
                A.build_modes(seed, 3, count)
                A.propagate_frames(0, count)
                B.build_potentials(pos, Z, slice_axis)
                B.propagate_frames(0, count)
            else:
                A.build_modes(seed, 3, 1)
                A.propagate_frame(0)
                B.build_potential(pos[0], Z, slice_axis)
                B.propagate_frame(0)
            a, b = A.wavefunction()[:, :count], B.wavefunction()[:, :count]
            assert np.isfinite(a).all() and np.abs(a).max() > 0
            assert np.array_equal(bits(a), bits(b)), (fb, count, rel_l2(a, b))
            assert np.array_equal(bits(A.transmission()), bits(B.transmission()))
            if count > 1:                                           # the frames differ from one another
                assert not np.array_equal(a[:, 0], a[:, 1])
        finally:
            A.close()
            B.close()


@pytest.mark.parametrize("dynamic", [True, False])
def test_random_access(ps, dynamic):
    """frame c built alone (the kernel's tile of 2 frames) is frame c built inside a batch of 11 (slots in both tiles of 8), bit for bit, and the same again when
    asked twice; a Trajectory-style build on the same handle in between leaves the structure and the modes as they are"""
    pm = modes(*SHAPES[0])
    seed = pm.seed
    A = make_engine(ps, pm, n_frames=11, frame_batch=11, dynamic=dynamic)
    B = make_engine(ps, pm, n_frames=4, frame_batch=11, dynamic=dynamic)
    try:
        A.build_modes(seed, 2, 11)
        A.propagate_frames(0, 11)
        batch = A.wavefunction()
        for slot, c in ((0, 2), (3, 5), (9, 11)):
            B.build_modes(seed, c, 1)
            B.propagate_frames(slot % 4, 1)
            alone = B.wavefunction()[:, slot % 4]
            assert np.array_equal(bits(alone), bits(batch[:, slot])), (dynamic, c)
        assert not np.array_equal(batch[:, 0], batch[:, 9])
        B.build_potentials(np.zeros((2, 1, 3)) + 1.2, np.array([79], dtype=np.int32))
        B.build_modes(seed, 5, 1)
        B.propagate_frames(2, 1)
        assert np.array_equal(bits(B.wavefunction()[:, 2]), bits(batch[:, 3]))
    finally:
        A.close()
        B.close()


# ---- the calculator ----------------------------------------------------------------------------------------
def _no_atom_near_a_slice_edge(ps, pm, tr):
    """on the CPU: no atom of any definition frame within 1e-9 A of a slice edge, so that the 1e-13 A between the device's
    positions and the definition's cannot move an atom to another slice"""
    from pyslice_amd.potentials import slice_edges
    zs = ps.gridFromTrajectory(pm, 0.1, 1.0)[2]
    lo, hi = slice_edges(zs)
    edges = np.unique(np.concatenate([lo, hi]))
    z = tr.positions[..., 2]
    assert z.min() > lo[0] + 1e-9 and z.max() < hi[-1] - 1e-9
    assert np.abs(z[..., None] - edges).min() > 1e-9


@pytest.mark.parametrize("shape", SHAPES)
def test_run_matches_the_definition(ps, shape):
    """MultisliceCalculator.run() on the PhononModes against run() on its to_trajectory(): 5 frames, 2 probes, rel-L2 <= 1e-4 on the
    wavefunctions (the parity contract)"""
    pm, tr = modes(*shape), materialised(*shape)
    _no_atom_near_a_slice_edge(ps, pm, tr)
    out = []
    for source in (pm, tr):
        calc = ps.MultisliceCalculator(progress=False, frame_batch=2, dtype="complex64")
        calc.setup(source, aperture=30.0, voltage_eV=EV, slice_thickness=1.0, probe_positions=PP[:2])
        assert (calc.nx, calc.ny, calc.nz) == shape
        wf = calc.run()
        out.append(npy(wf.wavefunction_data))
        assert np.allclose(wf.time, np.arange(5) * pm.timestep)
    assert out[0].shape == (2, 5) + shape[:2] + (1,)
    err = rel_l2(out[0], out[1])
    print(f"{shape}: run() on PhononModes against its to_trajectory(): rel-L2 {err:.3e}")
    assert err <= 1e-4
    assert rel_l2(out[1][:, 0], out[1][:, 1]) > 1e-3               # (the frames are not one another)


def _mode_runs(ps, shape, run, **kw):
    pm, tr = modes(*shape), materialised(*shape)
    _no_atom_near_a_slice_edge(ps, pm, tr)
    out = []
    for source in (pm, tr):
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
    """probe batches outside, frames inside: every probe batch regenerates the five frames by index"""
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


def test_tacaw_peaks_where_tau_says(ps):
    """a dynamic record of T = 16 frames of one mode with tau = 3/16 cycles per frame (timestep 1): the strongest bin of the TACAW
    spectrum away from frequency zero is +-3/16, and the two of them hold nearly all of it (displacements of 0.01 A: first order)"""
    from pyslice_amd.phonons import PhononModes
    base = modes(*SHAPES[0])
    W = np.zeros((1, 3, 3), dtype=complex)
    W[0, :, 0] = [0.01, 0.01j, -0.01]
    pm = PhononModes(base.atom_types, base.positions, base.box_matrix, base.basis_index, [[0.31, 0.17, 0.0]], [3 / 16], W, 16, seed=4)
    calc = ps.MultisliceCalculator(progress=False, frame_batch=4)
    calc.setup(pm, aperture=30.0, voltage_eV=EV, slice_thickness=1.0, probe_positions=PP[:2])
    tac = ps.TACAWData(calc.run())
    f = npy(tac.frequencies)
    spec = npy(tac.spectrum(None))
    assert f.shape == spec.shape == (16,)
    away = np.abs(f) > 1e-12
    peak = f[away][np.argmax(spec[away])]
    share = spec[np.isclose(np.abs(f), 3 / 16)].sum() / spec[away].sum()
    print(f"TACAW of a tau = 3/16 record: strongest bin at {peak:+.4f}, {share:.4f} of the non-zero-frequency intensity at +-3/16")
    assert np.isclose(abs(peak), 3 / 16) and share > 0.9


# ---- refusals and teardown ---------------------------------------------------------------------------------
def test_refusals(ps):
    pm = modes(*SHAPES[0])
    eng = make_engine(ps, pm, structure=False)
    try:
        with pytest.raises(ValueError, match="msl_set_structure"):
            put_modes(eng, pm)
        eng.set_structure(pm.positions, pm.atom_types, np.zeros(N_ATOMS))
        with pytest.raises(ValueError, match="msl_set_modes"):
            eng.build_modes(0, 0, 1)
        with pytest.raises(ValueError, match="msl_set_modes"):
            eng.mode_positions(0, 0)
        b = pm.basis_index.copy()
        for bad in (3, -1):
            b[17] = bad
            with pytest.raises(ValueError, match="basis index"):
                eng.set_modes(b, pm.wavevectors, pm.tau, pm.displacements)
        with pytest.raises(ValueError, match="atoms, the structure has"):
            eng.set_modes(pm.basis_index[:-1], pm.wavevectors, pm.tau, pm.displacements)
        tau = pm.tau.copy()
        for bad in (-0.25, np.nan, np.inf):
            tau[5] = bad
            with pytest.raises(ValueError, match="tau"):
                eng.set_modes(pm.basis_index, pm.wavevectors, tau, pm.displacements)
        q = pm.wavevectors.copy()
        q[3, 1] = np.inf
        with pytest.raises(ValueError, match="wave vector"):
            eng.set_modes(pm.basis_index, q, pm.tau, pm.displacements)
        W = pm.displacements.copy()
        W[2, 1, 0] = complex(0.0, np.nan)
        with pytest.raises(ValueError, match="displacement vector of mode 2"):
            eng.set_modes(pm.basis_index, pm.wavevectors, pm.tau, W)
        with pytest.raises(ValueError, match="n_modes"):
            eng.set_modes(pm.basis_index, pm.wavevectors[:0], pm.tau[:0], pm.displacements[:0])
        with pytest.raises(ValueError, match="msl_set_modes"):                 # nothing valid was set so far
            eng.build_modes(0, 0, 1)
        put_modes(eng, pm)
        before = eng.mode_positions(5, 3)
        with pytest.raises(ValueError, match="tau"):                           # a refused call leaves the resident modes as they were
            eng.set_modes(pm.basis_index, pm.wavevectors, tau, pm.displacements)
        assert np.array_equal(bits(eng.mode_positions(5, 3)), bits(before))
        eng.build_modes(0, 0, 1)
        for first, count in ((0, 0), (0, 5), (-1, 1), (2 ** 31 - 3, 4)):
            with pytest.raises(ValueError):
                eng.build_modes(0, first, count)
        with pytest.raises(ValueError):
            eng.mode_positions(0, 2 ** 31)
        eng.build_modes(0, 2 ** 31 - 4, 4)                                      # the last frames of a dynamic record
        put_modes(eng, pm, dynamic=False)
        eng.build_modes(0, 2 ** 31 - 3, 4)                                      # snapshots: any index below 2^63
        eng.synchronize()
        eng.set_structure(pm.positions, pm.atom_types, np.zeros(N_ATOMS))       # a new structure drops the modes
        with pytest.raises(ValueError, match="msl_set_modes"):
            eng.build_modes(0, 0, 1)
        eng.build_thermal(0, 0, 4)                                              # ... and is a structure
        eng.synchronize()
    finally:
        eng.close()


def test_modes_teardown_returns_all_device_memory(ps):
    """set_structure / set_modes (twice) / build_modes / mode_positions / destroy, three times in one process (the pattern of
    test_structure_teardown_returns_all_device_memory): free device memory after the third cycle is within the smallest resident
    buffer of the modes (tau of 2^14 modes: 128 KiB; q is 384 KiB, C 512 KiB, the basis indices of 2^18 atoms 1 MiB, W 2.25 MiB) of
    the value after the first."""
    import gc
    import torch
    from pyslice_amd.phonons import PhononModes
    from pyslice_amd.synthetic import box_for_grid
    n, M = 1 << 18, 1 << 14
    rng = np.random.default_rng(1)
    box = box_for_grid(64, 2, 0.1, 1.0)
    pm = PhononModes(np.array([14, 8])[rng.integers(0, 2, n)], rng.random((n, 3)) * np.diag(box), box, rng.integers(0, 3, n),
                     rng.random((M, 3)), rng.random(M), rng.standard_normal((M, 3, 3)) * (1e-4 + 0j), 2)
    torch.cuda.synchronize()

    def cycle():
        eng = make_engine(ps, pm, P=1, n_frames=2, frame_batch=2)
        put_modes(eng, pm)                                               # (a second set of modes replaces the first)
        eng.build_modes(1, 0, 2)
        eng.propagate_frames(0, 2)
        assert eng.mode_positions(1, 1).shape == (n, 3)
        eng.synchronize()
        eng.close()
        gc.collect()
        return torch.cuda.mem_get_info(0)[0]

    free = [cycle() for _ in range(3)]
    print(f"free device memory after each cycle: {free}, third - first = {free[2] - free[0]} bytes")
    assert abs(free[2] - free[0]) < M * 8, free
