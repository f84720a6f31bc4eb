"""Finite projection on the MI355X: the channel tables and the potential of msl_set_projection against the
float64 definitions of pyslice_amd/projection.py, the option switched off and back on, frozen phonons under it, and a run end to end.

Potential bound: on the same atoms the unchanged projection=None build is measured against oracle.potential (max-norm relative
error, as test_g4_potential); the finite build may miss finite_potential by twice that -- more terms per bin, fp32 row weights."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

EV = 100e3
POT_TOL = 1e-5        # tests/test_gpu_parity.py
WAVE_TOL = 1e-4       # tests/test_gpu_parity.py
TABLE_TOL = 2e-7      # test_g3_form_factor


def npy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


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


def make_engine(ps, nx, ny, nz, dz=0.5, d=0.1, **kw):
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import slice_edges
    eng = _native.Engine(nx, ny, nz, d, d, dz, wavelength(EV), interaction_sigma(EV), **kw)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(np.arange(nz) * dz))
    return eng


# ---- channel tables -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", [(32, 32), (45, 50)])
@pytest.mark.parametrize("R,J", [(1, 1), (2, 4)])
def test_channel_tables(ps, nx, ny, R, J):
    from pyslice_amd.projection import channel_tables
    species = [6, 14, 79]
    eng = make_engine(ps, nx, ny, 2, keep_potential=True)
    try:
        eng.set_projection(R, J)
        assert eng.get_projection() == (R, J)
        pos = np.tile(np.array([[0.5, 0.5, 0.3]]), (3, 1))
        eng.build_potential(pos, np.array(species, dtype=np.int32))
        nch = 3 * (2 * R + 1) * J
        got = eng.form_factors_finite(nch)
        want = channel_tables(species, nx, ny, 0.1, 0.1, 0.5, R, J)
        worst = max(rel_l2(got[c], want[c]) for c in range(nch))
        print(f"channel tables {nx}x{ny} R={R} J={J}: worst rel_l2 over {nch} channels {worst:.3e}")
        assert worst < TABLE_TOL
    finally:
        eng.close()


# ---- potential ----------------------------------------------------------------------------------------------------------------------

def _atoms(nx, ny, nz, n, species, J, seed, d=0.1, dz=0.5):
    """n random atoms inside the stack plus the placements that matter: on a node, on a slab edge, within h of lo[0] = 0 and within
    h of hi[nz-1] = nz dz -- columns (x, y, z), z the slice axis"""
    rng = np.random.default_rng(seed)
    top, h, e0 = nz * dz, dz / J, -dz / 2
    pos = rng.random((n, 3)) * [nx * d, ny * d, top]
    special = np.array([[0.31 * nx * d, 0.42 * ny * d, e0 + (J + 1) * h],                                   # on a node
                        [0.77 * nx * d, 0.18 * ny * d, e0 + dz],                                         # on a slab edge
                        [0.12 * nx * d, 0.66 * ny * d, 0.4 * h],                                         # within h of lo[0]
                        [0.55 * nx * d, 0.91 * ny * d, top - 0.3 * h]])                                  # within h of hi[nz-1]
    pos = np.vstack([pos, special])
    Z = np.array(species)[rng.integers(0, len(species), len(pos))]
    return pos, Z


# (nx, ny, nz, reach in A, J, slice_axis, atoms, species): dz = 0.5 A, so reach 0.5 -> R = 1, 1.0 -> R = 2, 4.5 -> R = 9 > nz
POTENTIAL_CASES = {
    "64x64x7_R2J4_tiled":      (64, 64, 7, 1.0, 4, 2, 40, [6, 14, 79]),          # Nyquist edge kernel, sparse: the tiled kernel
    "96x80x2_R1J1":            (96, 80, 2, 0.5, 1, 2, 30, [6, 79]),
    "45x50x1_R2J4":            (45, 50, 1, 1.0, 4, 2, 20, [14, 79]),             # odd lengths (chirp-z), one slice
    "45x50x7_R9J2_beyond":     (45, 50, 7, 4.5, 2, 2, 25, [6, 14, 79]),          # R > nz
    "64x64x2_R1J1_stream":     (64, 64, 2, 0.5, 1, 2, 256, [14]),                # 256 rows per bin: the persistent bf16 kernel
    "axis0_50x45_R2J4":        (50, 45, None, 0.2, 4, 0, 30, [6, 79]),           # slices along x: 50 slabs of 0.1 A, R = 2
}


@pytest.mark.parametrize("case", list(POTENTIAL_CASES))
def test_potential(ps, orc, case):
    from pyslice_amd import Projection
    from pyslice_amd.projection import finite_potential
    nx, ny, nz, reach, J, axis, n, species = POTENTIAL_CASES[case]
    if axis == 2:
        xs, ys, zs = np.arange(nx) * 0.1, np.arange(ny) * 0.1, np.arange(nz) * 0.5
        pos, Z = _atoms(nx, ny, nz, n, species, J, seed=nx + nz)
    else:
        # the reference's axis rule: the slices follow xs, the in-plane coordinates are columns 1, 2 on the (nx, ny) grid
        xs, ys, zs = np.arange(nx) * 0.1, np.arange(ny) * 0.1, np.arange(3) * 0.5
        p, Z = _atoms(nx, ny, nx, n, species, J, seed=7, dz=0.1)
        pos = np.ascontiguousarray(p[:, [2, 0, 1]])
    proj = Projection(reach=reach, nodes=J)
    base = npy(ps.Potential(xs, ys, zs, pos, list(Z), slice_axis=axis).array)
    want_inf = orc.potential(xs, ys, zs, pos, Z, axis)
    err_inf = np.abs(base - want_inf).max() / np.abs(want_inf).max()
    pot = ps.Potential(xs, ys, zs, pos, list(Z), slice_axis=axis, projection=proj)
    R = pot.projection_slices
    V = npy(pot.array)
    want = finite_potential(xs, ys, zs, pos, Z, R, J, axis)
    err = np.abs(V - want).max() / np.abs(want).max()
    note = "" if 2 * err_inf <= POT_TOL else f"  (the bound exceeds POT_TOL = {POT_TOL:g})"
    print(f"potential {case}: R={R} J={J}  infinite build vs oracle {err_inf:.3e}  finite build vs finite_potential {err:.3e}  bound {2 * err_inf:.3e}{note}")
    assert V.shape == want.shape and V.dtype == np.float64
    assert R == {0.5: 1, 1.0: 2, 4.5: 9, 0.2: 2}[reach]
    assert err < 2 * err_inf


# ---- the option off -----------------------------------------------------------------------------------------------------------------

def test_off_is_bit_for_bit_and_switching_rebuilds_the_tables(ps):
    from pyslice_amd.projection import channel_tables
    nx, ny, nz = 64, 48, 4
    pos, Z = _atoms(nx, ny, nz, 60, [6, 79], 2, seed=3)
    Z = Z.astype(np.int32)
    pp = np.array([[3.0, 2.0], [1.2, 4.1]])

    def run(eng):
        eng.build_potential(pos, Z)
        eng.set_probes(30.0, pp)
        eng.propagate()
        return eng.potential(), eng.exit_waves()
    A = make_engine(ps, nx, ny, nz, keep_potential=True, n_probes=2)
    B = make_engine(ps, nx, ny, nz, keep_potential=True, n_probes=2)
    try:
        B.set_projection(0, 1)
        Va, Ea = run(A)
        Vb, Eb = run(B)
        assert B.get_projection() == (0, 1) and A.get_projection() == (0, 1)
        assert np.array_equal(bits(Va), bits(Vb)) and np.array_equal(bits(Ea.view(np.float32)), bits(Eb.view(np.float32)))
        f_off = A.form_factors(2)
        # on -> off -> on: the tables of every build are those of its setting
        B.set_projection(2, 2)
        V1, E1 = run(B)
        t1 = B.form_factors_finite(2 * 5 * 2)
        assert rel_l2(t1, channel_tables([6, 79], nx, ny, 0.1, 0.1, 0.5, 2, 2)) < TABLE_TOL
        assert not np.array_equal(V1, Va)
        B.set_projection(0, 1)
        V2, E2 = run(B)
        assert np.array_equal(bits(B.form_factors(2)), bits(f_off))
        assert np.array_equal(bits(V2), bits(Va)) and np.array_equal(bits(E2.view(np.float32)), bits(Ea.view(np.float32)))
        B.set_projection(1, 2)
        run(B)
        assert rel_l2(B.form_factors_finite(2 * 3 * 2), channel_tables([6, 79], nx, ny, 0.1, 0.1, 0.5, 1, 2)) < TABLE_TOL
        B.set_projection(2, 2)
        V3, E3 = run(B)
        assert np.array_equal(bits(B.form_factors_finite(20)), bits(t1))
        assert np.array_equal(bits(V3), bits(V1)) and np.array_equal(bits(E3.view(np.float32)), bits(E1.view(np.float32)))
        for bad in ((1, 0), (1, 17), (-1, 1), (33, 1)):
            with pytest.raises(ValueError):
                B.set_projection(*bad)
        assert B.get_projection() == (2, 2)
    finally:
        A.close()
        B.close()


def test_absorption_and_projection_refuse_each_other(ps):
    eng = make_engine(ps, 32, 32, 2)
    try:
        eng.set_absorption(np.full(103, 0.08), True)
        with pytest.raises(NotImplementedError, match="msl_set_projection"):
            eng.set_projection(1, 1)
        eng.set_absorption(None)
        eng.set_projection(1, 1)
        with pytest.raises(NotImplementedError, match="finite projection"):
            eng.set_absorption(np.full(103, 0.08), True)
    finally:
        eng.close()


def test_non_uniform_slices_are_refused_at_the_build(ps):
    eng = make_engine(ps, 32, 32, 4)
    try:
        eng.set_slices(np.array([0.0, 0.25, 0.75, 1.5]), np.array([0.25, 0.75, 1.5, 2.0]))
        eng.set_projection(1, 1)
        with pytest.raises(NotImplementedError, match="uniform slices only"):
            eng.build_potential(np.array([[1.0, 1.0, 0.5]]), np.array([6], dtype=np.int32))
    finally:
        eng.close()


# ---- frozen phonons -----------------------------------------------------------------------------------------------------------------

def test_frozen_phonons_under_projection(ps):
    """two configurations of one frame batch: the transmission stacks against exp(i sigma finite_potential(configuration(k))), to the
    1e-4 the transmission downloads of tests/test_gpu_parity.py are held to"""
    from pyslice_amd import _native, Projection
    from pyslice_amd.multislice import interaction_sigma
    from pyslice_amd.projection import finite_potential
    from pyslice_amd.synthetic import box_for_grid
    from pyslice_amd.thermal import FrozenPhonons
    nx, ny, nz = 48, 40, 5
    box = box_for_grid(nx, nz, 0.1, 0.5, ny)
    rng = np.random.default_rng(17)
    n = 50
    pos = np.array([0.0, 0.0, 0.6]) + rng.random((n, 3)) * [box[0, 0], box[1, 1], box[2, 2] - 1.2]
    fp = FrozenPhonons(np.array([14, 79])[rng.integers(0, 2, n)], pos, box, rng.random(n) * 0.08, 2, seed=5)
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64", frame_batch=2, projection=Projection(reach=1.0, nodes=3))
    calc.setup(fp, aperture=30.0, voltage_eV=EV, probe_positions=[(2.0, 2.0)])
    calc.run()
    eng = calc._engine
    assert eng.frame_batch == 2 and (calc.nx, calc.ny, calc.nz) == (nx, ny, nz)
    assert eng.get_projection() == (calc.projection_slices, 3)
    for k in range(2):
        eng.select_batch_slot(k)
        t = eng.download(_native.BUF_TRANSMISSION, np.complex64, (nz, nx, ny))
        V = finite_potential(calc.xs, calc.ys, calc.zs, fp.configuration(k), fp.atom_types, calc.projection_slices, 3)
        err = rel_l2(t, np.exp(1j * interaction_sigma(EV) * np.moveaxis(V, 2, 0)))
        print(f"frozen phonons, configuration {k}: transmission rel_l2 {err:.3e}")
        assert err < 1e-4


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_run_equals_propagate_over_the_uploaded_finite_potential(ps):
    from pyslice_amd import Projection
    from pyslice_amd.projection import finite_potential
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(64, 8, 1, density=0.1, seed=9)
    pp = [(3.0, 3.0), (1.2, 4.4), (5.1, 0.7), (0.0, 6.0)]
    calc = ps.MultisliceCalculator(progress=False, projection=Projection(reach=1.0, nodes=4))
    calc.setup(tr, aperture=30.0, voltage_eV=EV, probe_positions=pp)
    assert (calc.nx, calc.ny, calc.nz) == (64, 64, 8)
    got = npy(calc.run().wavefunction_data).reshape(4, 64, 64)
    V = finite_potential(calc.xs, calc.ys, calc.zs, tr.positions[0], tr.atom_types, calc.projection_slices, 4)
    pot = ps.Potential(calc.xs, calc.ys, calc.zs, tr.positions[0], list(tr.atom_types))
    pot.array = V
    ex = npy(ps.Propagate(ps.create_batched_probes(ps.Probe(calc.xs, calc.ys, 30.0, EV), pp), pot))
    want = np.fft.fftshift(np.fft.fft2(ex, axes=(1, 2)), axes=(1, 2))
    err = rel_l2(got, want)
    # and the option does something: the infinite projection of the same frame is another wave
    base = ps.MultisliceCalculator(progress=False)
    base.setup(tr, aperture=30.0, voltage_eV=EV, probe_positions=pp)
    differs = rel_l2(npy(base.run().wavefunction_data).reshape(4, 64, 64), want)
    print(f"end to end: run(projection) vs Propagate(finite_potential) {err:.3e}; the infinite projection differs by {differs:.3e}")
    assert err < WAVE_TOL
    assert differs > 10 * WAVE_TOL
