"""Element maps on the MI355X: the weight stack the device builds, the slice loop's reduction and run_element_maps(), against the
float64 definition (pyslice_amd/ionization.py) carried through the float64 oracle.

Cells: 10 atoms of Si and O in 4 slices of 0.875 A, 0.1 A pixels, 100 kV, 30 mrad; one atom exactly on a slice boundary (it belongs
to the slice that begins there), one 0.05 A from the cell edge (its Gaussian wraps), slice 1 without atoms.  Grids 64 x 64 (power of
two), 48 x 40 (mixed radix, non-square), 45 x 64 (odd length: pitch padding, the 8-byte loads).  3 probes at a probe batch of 2: the
last batch is padded.  Channels Si w = 0.15, O w = 0.4, Si w = 0.4 and Au, which the cells do not hold.  Two frames.

Bounds, from the project's contracts and not from the kernel.  Weight stack: the potential contract, 1e-5 of the maximum of the
float64 stack of the channel (W is the potential build with another table).  Per-slice signals, per incident electron: the waves are
held to a rel-L2 of 1e-4 (the wavefunction contract), so |psi|^2 moves by 2e-4 of its sum, which is at most the incident one, and W
by 1e-5 of its maximum:  |I - I_want| <= (2e-4 + 1e-5) max W_e -- the bound tests/test_gpu_tds.py puts on the same kind of sum, with
the weights' own term where they are the float64 ones (the engine-level test feeds the device's t and W: 2e-4 max W_e).  The
reduction alone is held tighter, against the float64 sum of the very waves it read: 1e-6 of sum |psi_0|^2 max W, a float32 partial
of 1024 non-negative terms being good to about sqrt(1024) 2^-24 = 2e-6 of its own sum.  Every figure is printed before it is
asserted; those of the MI355X are in profiles/element_signals.txt (at most 3.9e-7 of the largest signal of a case)."""
import functools

import numpy as np
import pytest

from oracle import multislice_oracle as orc
from test_gpu_absorptive import stack_from_tables
from test_gpu_tds import check_streaming, streaming_probe_count

pytestmark = pytest.mark.gpu

EV = 100e3
NZ = 4
GRIDS = [(64, 64), (48, 40), (45, 64)]
ODD_NY = (64, 45)                           # rows of odd length: the last pixel pair of a row has one pixel
U = {14: 0.078, 8: 0.09}
WAVE, POT = 1e-4, 1e-5                      # the wavefunction and the potential contract


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def channels(n=4):
    from pyslice_amd.ionization import Ionization
    four = [Ionization(14, 0.15, 0.7), Ionization(8, 0.4, 1.3), Ionization(14, 0.4, 0.7, name="Si-L"), Ionization(79, 0.3)]
    more = [Ionization(8, 0.2, 0.5, name="O-2"), Ionization(14, 0.25, 2.0, name="Si-3"), Ionization(8, 0.3, 1.0, name="O-3"),
            Ionization(14, 0.5, 0.1, name="Si-4")]
    return (four + more)[:n]


@functools.lru_cache(maxsize=None)
def cell(nx, ny):
    """box, grid axes, positions (2 frames, 10, 3), Z and the 3 probe positions of a grid; read-only"""
    from pyslice_amd.potentials import slice_edges
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(nx, NZ, 0.1, 1.0, ny)
    lx, ly, lz = box[0, 0], box[1, 1], box[2, 2]
    xs, ys, zs = np.linspace(0, lx, nx, endpoint=False), np.linspace(0, ly, ny, endpoint=False), np.linspace(0, lz, NZ, endpoint=False)
    lo, hi = slice_edges(zs)
    rng = np.random.default_rng(1000 * nx + ny)
    n = 10
    pos = rng.random((n, 3)) * np.array([lx, ly, 1.0])
    for i, s in enumerate([2, 0, 0, 2, 3, 3, 0, 2, 3, 3]):     # slice 1 stays empty
        pos[i, 2] = lo[s] + (0.1 + 0.8 * rng.random()) * (hi[s] - lo[s])
    pos[0, 2] = lo[2]                                           # exactly on a slice boundary
    pos[1, 0] = 0.05                                            # within a width of the cell edge
    Z = np.array([14, 8] * (n // 2), dtype=np.int32)
    frames = np.stack([pos, pos + np.concatenate([0.03 * rng.standard_normal((n, 2)), np.zeros((n, 1))], axis=1)])
    frames[1, 1, 0] = lx - 0.05                                 # (the other side of the edge)
    pp = [(float(pos[0, 0]), float(pos[0, 1])), (0.1, float(pos[1, 1])), (0.37 * lx, 0.61 * ly)]
    out = dict(box=box, xs=xs, ys=ys, zs=zs, frames=frames, Z=Z, pp=pp, dz=zs[1] - zs[0])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def probes64(c):
    return orc.batched_probes(orc.probe_array(c["xs"], c["ys"], 30.0, EV), c["xs"], c["ys"], c["pp"])


def propagator(c):
    from pyslice_amd.tilt import tilted_propagator
    xs, ys = c["xs"], c["ys"]
    return tilted_propagator(len(xs), len(ys), xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), c["dz"], None)


def elastic_t(c, pos):
    V = np.moveaxis(orc.potential(c["xs"], c["ys"], c["zs"], pos, c["Z"]), 2, 0)
    return np.exp(1j * orc.interaction_sigma(EV) * V)


def want_signal(c, chs, frames, transmission=elastic_t):
    """(I (P, E, nz) float64, the mean over the frames; max W per channel over the frames)"""
    from pyslice_amd.ionization import ionization_signal, ionization_weights
    I, wmax = 0.0, np.zeros(len(chs))
    for pos in frames:
        W = ionization_weights(chs, c["xs"], c["ys"], c["zs"], pos, c["Z"])
        I = I + ionization_signal(probes64(c), transmission(c, pos), W, propagator(c))[0]
        wmax = np.maximum(wmax, np.abs(W).max(axis=(1, 2, 3)))
    return I / len(frames), wmax


@functools.lru_cache(maxsize=None)
def want_trajectory(nx, ny):
    c = cell(nx, ny)
    I, wmax = want_signal(c, channels(), c["frames"])
    I.setflags(write=False)
    return I, wmax


def check(name, got, want, wmax):
    bound = (2.0 * WAVE + POT) * wmax[None, :, None]
    err = np.abs(got - want)
    print(f"element maps {name}: worst |I - I_want| / bound {(err / np.maximum(bound, 1e-300))[:, wmax > 0].max():.3e}, relative to the "
          f"largest I {err.max() / want.max():.3e}, largest I {want.max():.4e}, max W {wmax.max():.3e}")
    assert got.shape == want.shape
    assert (err <= bound).all()
    assert want.max() > 1e-4


def make_engine(ps, c, chs, n_probes=3, **kw):
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    xs, ys, zs = c["xs"], c["ys"], c["zs"]
    eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], c["dz"], orc.wavelength(EV), orc.interaction_sigma(EV),
                         n_probes=n_probes, **kw)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(zs))
    if chs is not None:
        eng.set_ionization(chs)
    return eng


def scan(ps, grid, source, **kw):
    c = cell(*grid)
    calc = ps.MultisliceCalculator(device=0, progress=False, ionization=channels(), probe_batch=2, **kw)
    calc.setup(source, aperture=30.0, voltage_eV=EV, probe_positions=c["pp"], sampling=0.1, slice_thickness=1.0)
    assert (calc.nx, calc.ny, calc.nz) == (*grid, NZ) and calc._engine.n_probes == 2 and calc._engine.frame_batch == 1
    return calc, calc.run_element_maps()


def trajectory(ps, c):
    return ps.Trajectory(c["Z"], c["frames"], np.zeros_like(c["frames"]), c["box"], 0.005)


@pytest.mark.parametrize("grid", GRIDS + [ODD_NY])
def test_weight_stack(ps, grid):
    from pyslice_amd.ionization import ionization_weights
    c, chs = cell(*grid), channels()
    eng = make_engine(ps, c, chs)
    eng.build_potential(c["frames"][0], c["Z"])
    assert eng.buffer_bytes(18) == 4 * NZ * grid[0] * grid[1] * 4
    W = eng.ionization_weight().astype(np.float64)
    want = ionization_weights(chs, c["xs"], c["ys"], c["zs"], c["frames"][0], c["Z"])
    for e in range(3):
        err = np.abs(W[e] - want[e]).max() / np.abs(want[e]).max()
        print(f"element maps weights {grid} channel {e}: max error over max W {err:.2e} (1e-5), max W {np.abs(want[e]).max():.3e}")
        assert err <= POT, e
    assert not W[3].any() and not want[3].any()                 # the absent element: zeros, not an error
    assert not want[:, 1].any() and np.abs(W[:, 1]).max() <= POT * np.abs(want).max()      # the empty slice
    eng.set_ionization(None)
    assert eng.buffer_bytes(18) == 0
    with pytest.raises(RuntimeError):
        eng.ionization_fetch()


@pytest.mark.parametrize("grid", GRIDS + [ODD_NY])
def test_trajectory_run(ps, grid):
    c = cell(*grid)
    want, wmax = want_trajectory(*grid)
    calc, res = scan(ps, grid, trajectory(ps, c))
    check(f"trajectory {grid}", res.per_slice, want, wmax)
    assert not res.per_slice[:, 3].any()                        # the absent element is exactly zero
    assert not res.per_slice[:, :, 1].any() or np.abs(res.per_slice[:, :, 1]).max() <= POT * wmax.max()     # the empty slice
    assert np.array_equal(res.cumulative()[..., -1], res.signals) and res.names == ["Si", "O", "Si-L", "Au"]
    assert res.image("Si").shape == (3, 3) and res.depth_profile("O", 1).shape == (NZ,)
    # two widths of one element differ, and the probe on the Si column sees more Si than the one between the atoms
    assert np.abs(res.per_slice[:, 0] - res.per_slice[:, 2]).max() > 10 * (2.0 * WAVE + POT) * wmax[0]
    # a second run gives the same bits; so does one whole-scan batch (every image is reduced on its own)
    _, again = scan(ps, grid, trajectory(ps, c))
    assert again.per_slice.tobytes() == res.per_slice.tobytes()
    whole = ps.MultisliceCalculator(device=0, progress=False, ionization=channels())
    whole.setup(trajectory(ps, c), aperture=30.0, voltage_eV=EV, probe_positions=c["pp"], sampling=0.1, slice_thickness=1.0)
    assert whole.run_element_maps().per_slice.tobytes() == res.per_slice.tobytes()


@pytest.mark.parametrize("grid", GRIDS)
def test_frozen_phonons_run(ps, grid):
    c = cell(*grid)
    src = ps.FrozenPhonons(c["Z"], c["frames"][0], c["box"], {14: 0.03, "O": 0.04}, 2, seed=7)
    calc, res = scan(ps, grid, src)
    frames = [calc._engine.thermal_positions(src.seed, k) for k in range(2)]
    assert np.abs(frames[0] - src.configuration(0)).max() <= 1e-12 and np.abs(frames[0] - frames[1]).max() > 1e-3
    want, wmax = want_signal(c, channels(), frames)
    check(f"frozen phonons {grid}", res.per_slice, want, wmax)
    assert not res.per_slice[:, 3].any() and res.n_frames == 2


@pytest.mark.parametrize("grid", GRIDS)
def test_absorptive_run(ps, grid):
    from pyslice_amd.absorptive import AbsorptivePotential, absorptive_tables, absorptive_transmission
    c = cell(*grid)
    xs, ys = c["xs"], c["ys"]
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    q2 = np.fft.fftfreq(len(xs), dx)[:, None] ** 2 + np.fft.fftfreq(len(ys), dy)[None, :] ** 2
    tables = {Z: absorptive_tables(orc.form_factor(q2, Z), q2, U[Z], dx, dy) for Z in (8, 14)}

    def transmission(c, pos):
        Vbar, Om = (stack_from_tables(xs, ys, c["zs"], pos, c["Z"], {Z: tables[Z][k] for Z in (8, 14)}) for k in (0, 1))
        return absorptive_transmission(Vbar, Om, orc.interaction_sigma(EV))
    src = AbsorptivePotential(c["Z"], c["frames"][0], c["box"], U)
    calc, res = scan(ps, grid, src)
    want, wmax = want_signal(c, channels(), [c["frames"][0]], transmission)
    check(f"absorptive {grid}", res.per_slice, want, wmax)
    # the weights are those of the static positions: only the wave differs from the elastic run, and it loses intensity
    elastic = want_signal(c, channels(), [c["frames"][0]])[0]
    assert res.per_slice[:, :3, -1].sum() < elastic[:, :3, -1].sum()


@pytest.mark.parametrize("grid, n", [(GRIDS[0], 8), (GRIDS[2], 8), (GRIDS[1], 1), (GRIDS[2], 1), (GRIDS[1], 5), (ODD_NY, 4), (ODD_NY, 2)])
def test_engine_loop_for_one_to_eight_channels(ps, grid, n, monkeypatch):
    """the loop and the reduction alone, fed the device's own t and W; the exit waves are the two-pass loop's, bit for bit"""
    from pyslice_amd.ionization import ionization_signal
    c, chs = cell(*grid), channels(n)
    eng = make_engine(ps, c, chs)
    eng.build_potential(c["frames"][0], c["Z"])
    eng.set_probes(30.0, np.asarray(c["pp"]))
    eng.propagate()
    got = np.moveaxis(eng.ionization_fetch(), 0, -1)            # (P, E, nz)
    t, W = eng.transmission().astype(np.complex128), eng.ionization_weight().astype(np.float64)
    ref, _ = ionization_signal(probes64(c), t, W, propagator(c))
    check(f"engine {grid} x {n}", got, ref, np.abs(W).max(axis=(1, 2, 3)) * (2.0 * WAVE) / (2.0 * WAVE + POT))
    assert got.shape == (3, n, NZ)
    ex = eng.exit_waves()
    eng.propagate()
    assert np.moveaxis(eng.ionization_fetch(), 0, -1).tobytes() == got.tobytes() and eng.exit_waves().tobytes() == ex.tobytes()
    assert np.moveaxis(eng.ionization_fetch(B=2), 0, -1).tobytes() == got[:2].tobytes()
    # the stand-alone reduction of the exit waves against slice 0 is the float64 sum of the downloaded waves
    alone, _ = eng.ionization_reduce(0, 1)
    ref_alone = np.einsum("pxy,exy->pe", np.abs(ex.astype(np.complex128)) ** 2, W[:, 0])
    n0 = (np.abs(probes64(c)) ** 2).sum(axis=(1, 2))
    assert np.abs(alone - ref_alone).max() <= 1e-6 * n0.max() * np.abs(W[:, 0]).max()
    # the same handle without ionisation, forced to the two-pass loop: the same exit waves
    monkeypatch.setenv("MSL_DEBUG", "1")
    monkeypatch.setenv("MSL_SLICE_PATH", "2")
    two = make_engine(ps, c, None)
    two.build_potential(c["frames"][0], c["Z"])
    two.set_probes(30.0, np.asarray(c["pp"]))
    two.propagate()
    assert two.exit_waves().tobytes() == ex.tobytes()
    assert two.transmission().tobytes() == eng.transmission().tobytes()
    monkeypatch.delenv("MSL_SLICE_PATH")
    monkeypatch.delenv("MSL_DEBUG")
    # cleared: the handle runs its own loop again, as one that never had the setting
    eng.set_ionization(None)
    eng.build_potential(c["frames"][0], c["Z"])
    eng.propagate()
    fresh = make_engine(ps, c, None)
    fresh.build_potential(c["frames"][0], c["Z"])
    fresh.set_probes(30.0, np.asarray(c["pp"]))
    fresh.propagate()
    assert eng.exit_waves().tobytes() == fresh.exit_waves().tobytes()


@pytest.mark.parametrize("which", ["odd", "ragged"])
def test_reduction_streams_chunks_of_images_with_a_short_last_chunk(ps, which):
    """64 x 45: 64 x 23 = 1472 pixel pairs, 3 tiles of 512 with a partial last one; 5 channels in the 8 slots of the kernel"""
    c, chs = cell(*ODD_NY), channels(5)
    P = streaming_probe_count(3, which)
    eng = make_engine(ps, c, chs, n_probes=P)
    eng.build_potential(c["frames"][0], c["Z"])
    eng.set_probes(30.0, np.asarray([c["pp"][p % 3] for p in range(P)]))
    eng.propagate()
    n0 = (np.abs(probes64(c)) ** 2).sum(axis=(1, 2))
    check_streaming(eng, eng.ionization_reduce, eng.ionization_weight().astype(np.float64)[:, 0], n0)


def test_smatrix_build_under_ionization_runs_the_plain_loop_and_keeps_the_sums(ps, monkeypatch):
    """msl_smatrix_build goes through the slice loop too: with the setting on it issues the launches of a handle without it (the
    two-pass loop the setting forces) and leaves the sums of the last probe loop where they are"""
    c = cell(*GRIDS[1])
    eng = make_engine(ps, c, channels(3), n_frames=1)
    eng.build_potential(c["frames"][0], c["Z"])
    eng.set_probes(30.0, np.asarray(c["pp"]))
    eng.propagate()
    sums, c0 = eng.ionization_fetch(), eng.counters()
    n_beams = eng.smatrix_begin((1, 1), 30.0)
    eng.smatrix_build()
    S, c1 = eng.smatrix(), eng.counters()
    assert eng.ionization_fetch().tobytes() == sums.tobytes()
    monkeypatch.setenv("MSL_DEBUG", "1")
    monkeypatch.setenv("MSL_SLICE_PATH", "2")
    plain = make_engine(ps, c, None, n_frames=1)
    plain.build_potential(c["frames"][0], c["Z"])
    plain.set_probes(30.0, np.asarray(c["pp"]))
    p0 = plain.counters()
    assert plain.smatrix_begin((1, 1), 30.0) == n_beams
    plain.smatrix_build()
    p1 = plain.counters()
    assert plain.smatrix().tobytes() == S.tobytes() and np.abs(S).max() > 0
    for k in ("row_launches", "col_launches", "slice_kernel_launches", "slice_steps", "algorithmic_bytes"):
        assert c1[k] - c0[k] == p1[k] - p0[k], k


def test_without_ionization_the_calculator_runs_as_before(ps):
    from pyslice_amd.stem_data import Detector
    c = cell(*GRIDS[1])
    out = []
    for kw in ({}, dict(ionization=None)):
        calc = ps.MultisliceCalculator(device=0, progress=False, detectors=[Detector("d", inner=30.0, outer=90.0)], **kw)
        calc.setup(trajectory(ps, c), aperture=30.0, voltage_eV=EV, probe_positions=c["pp"], sampling=0.1, slice_thickness=1.0)
        out.append(calc.run_detectors().signals)
        assert calc._engine.buffer_bytes(18) == 0
    assert out[0].tobytes() == out[1].tobytes()


def test_set_ionization_refusals(ps):
    from pyslice_amd import _native
    from pyslice_amd.absorptive import AbsorptivePotential
    from pyslice_amd.tds import tds_members
    from pyslice_amd.stem_data import Detector
    c = cell(*GRIDS[1])
    eng = make_engine(ps, c, None)

    def call(n, Z, w, cs):
        Z, w, cs = np.asarray(Z, dtype=np.int32), np.asarray(w, dtype=np.float64), np.asarray(cs, dtype=np.float64)
        return eng._lib.msl_set_ionization(eng._h, n, Z.ctypes.data, w.ctypes.data, cs.ctypes.data)
    assert call(9, [14] * 9, [0.2] * 9, [1.0] * 9) == _native.MSL_ERR_INVALID
    for w in (0.0, -0.1, np.inf, np.nan):
        assert call(1, [14], [w], [1.0]) == _native.MSL_ERR_INVALID
    assert call(1, [14], [0.2], [-1.0]) == _native.MSL_ERR_INVALID
    assert call(1, [0], [0.2], [1.0]) == _native.MSL_ERR_INVALID
    assert call(8, [14] * 8, [0.2] * 8, [0.0] * 8) == _native.MSL_OK
    assert call(0, [14], [0.2], [1.0]) == _native.MSL_OK and eng.buffer_bytes(18) == 0
    # one per-slice reduction per handle: with tds set, and the reverse
    ap = AbsorptivePotential(c["Z"], c["frames"][0], c["box"], U)
    bits = tds_members([Detector("d", inner=40.0, outer=120.0)], *GRIDS[1], 0.1, 0.1, orc.wavelength(EV))
    eng.set_absorption(ap.u_by_Z, True)
    eng.set_tds(bits, 1)
    assert call(1, [14], [0.2], [1.0]) == _native.MSL_ERR_STATE
    eng.set_tds(None)
    assert call(1, [14], [0.2], [1.0]) == _native.MSL_OK
    assert eng._lib.msl_set_tds(eng._h, bits.ctypes.data, 1) == _native.MSL_ERR_STATE
    with pytest.raises(RuntimeError):
        eng.propagate()                                         # the setting dropped the potential
    # a frame batch above one
    fb = make_engine(ps, c, None, frame_batch=2, n_frames=2)
    Z, w, cs = np.array([14], dtype=np.int32), np.array([0.2]), np.array([1.0])
    assert fb._lib.msl_set_ionization(fb._h, 1, Z.ctypes.data, w.ctypes.data, cs.ctypes.data) == _native.MSL_ERR_UNSUPPORTED
