"""Phonon modes on the host: the definition (pyslice_amd/phonons.py) -- validation, purity, the random stream, periodic dynamic
records, the variance identity, the thermal amplitudes of from_eigenvectors -- a travelling wave through the oracle's multislice and
TACAW transform, and the calls the calculator makes for a PhononModes in place of a Trajectory (RecordingEngine: no device)."""
import os

import numpy as np
import pytest

from oracle import multislice_oracle as orc
from pyslice_amd import phonons, thermal
from pyslice_amd.phonons import PhononModes
from recording_engine import RecordingEngine

EV = 100e3
EPS = 2.0 ** -52


def _structure(n_cells=(3, 2, 2), a=2.0, nb=2):
    """a simple lattice of n_cells cells with nb basis atoms each, in a box with vacuum along z"""
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in n_cells], indexing="ij"), axis=-1).reshape(-1, 3) * a
    basis = np.array([[0.3, 0.4, 1.5], [1.3, 1.4, 2.5]])[:nb]
    pos = (cells[:, None, :] + basis[None]).reshape(-1, 3)
    b = np.tile(np.arange(nb), len(cells))
    Z = np.array([14, 8])[b]
    box = np.diag([n_cells[0] * a, n_cells[1] * a, n_cells[2] * a + 3.0])
    return Z, pos, box, b


def _modes(box, M=6, nb=2, seed=5, T=16):
    """M modes commensurate with the box, tau = j / T (exact in binary for T = 16), complex W up to 0.05 A"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, (M, 3)) / np.diag(box)
    nu = rng.integers(1, T, M) / T
    W = (rng.standard_normal((M, nb, 3)) + 1j * rng.standard_normal((M, nb, 3))) * 0.02
    return q, nu, W


def _make(n_frames=16, seed=7, dynamic=True, **kw):
    Z, pos, box, b = _structure()
    q, nu, W = _modes(box)
    return PhononModes(Z, pos, box, b, q, nu, W, n_frames, seed=seed, dynamic=dynamic, **kw)


# ---- the input type ----------------------------------------------------------------------------------------
def test_members_and_trajectory():
    import pyslice_amd as ps
    pm = _make(n_frames=4, timestep=0.5)
    assert ps.PhononModes is PhononModes
    assert (pm.n_frames, pm.n_atoms, pm.n_modes, pm.n_basis, pm.timestep, pm.dynamic) == (4, 24, 6, 2, 0.5, True)
    assert np.array_equal(pm.box_tilts, [0.0, 0.0, 0.0])
    assert np.array_equal(pm.tau, pm.frequencies * 0.5) and pm.basis_index.dtype == np.int32
    tr = pm.to_trajectory()
    assert isinstance(tr, ps.Trajectory) and tr.positions.shape == (4, 24, 3) and tr.timestep == 0.5
    for c in range(4):
        assert np.array_equal(tr.positions[c], pm.configuration(c))
    assert np.array_equal(pm.to_trajectory([3, 1]).positions, tr.positions[[3, 1]])
    assert [len(v) for v in ps.gridFromTrajectory(pm)[:3]] == [len(v) for v in ps.gridFromTrajectory(tr)[:3]]


def test_validation_messages():
    Z, pos, box, b = _structure()
    q, nu, W = _modes(box)
    ok = lambda **k: PhononModes(**{**dict(atom_types=Z, positions=pos, box_matrix=box, basis_index=b, wavevectors=q, frequencies=nu,
                                           displacements=W, n_frames=4), **k})
    ok()
    for match, kw in ((r"box_matrix must be \(3, 3\)", dict(box_matrix=box[:2])),
                      ("atom_types must be 1D", dict(atom_types=Z[None])),
                      ("Atom count mismatch", dict(atom_types=Z[:-1], basis_index=b[:-1])),
                      ("positions must be", dict(positions=pos[None])),
                      ("positions must be finite", dict(positions=np.where(np.arange(24)[:, None] == 3, np.nan, pos))),
                      ("n_frames must be a positive integer", dict(n_frames=0)),
                      ("n_frames must be a positive integer", dict(n_frames=2.0)),
                      ("seed must be a non-negative 64-bit integer", dict(seed=-1)),
                      ("seed must be a non-negative 64-bit integer", dict(seed=2 ** 64)),
                      ("timestep must be finite and > 0", dict(timestep=0.0)),
                      (r"displacements must be \(modes >= 1, basis atoms >= 1, 3\)", dict(displacements=W[:, :, :2])),
                      (r"displacements must be \(modes >= 1", dict(displacements=W[:0], wavevectors=q[:0], frequencies=nu[:0])),
                      (r"wavevectors must be \(6, 3\)", dict(wavevectors=q[:5])),
                      (r"frequencies must be \(6,\)", dict(frequencies=nu[:5])),
                      ("every frequency must be finite and >= 0", dict(frequencies=-nu)),
                      ("every frequency must be finite and >= 0", dict(frequencies=nu * np.inf)),
                      ("wavevectors must be finite", dict(wavevectors=q * np.nan)),
                      ("displacements must be finite", dict(displacements=W * np.inf)),
                      (r"basis_index must be \(24,\)", dict(basis_index=b[:-1])),
                      ("basis_index must be integers", dict(basis_index=b.astype(float))),
                      (r"every index must be in \[0, 2\)", dict(basis_index=np.where(np.arange(24) == 5, 2, b))),
                      (r"every index must be in \[0, 2\)", dict(basis_index=np.where(np.arange(24) == 5, -1, b))),
                      ("dynamic record must be at most", dict(n_frames=2 ** 31 + 1))):
        with pytest.raises(ValueError, match=match):
            ok(**kw)
    ok(n_frames=2 ** 31 + 1, dynamic=False)
    ok(frequencies=np.zeros(6))                                  # a static mode is a mode (only from_eigenvectors refuses it)
    with pytest.raises(ValueError, match="frame index"):
        ok().configuration(-1)
    with pytest.raises(ValueError, match="below 2\\^31"):
        ok().configuration(2 ** 31)


# ---- purity and the stream ---------------------------------------------------------------------------------
def test_configuration_is_pure_and_reproducible():
    a, b = _make(), _make()
    first = a.configuration(5)
    a.configuration(2), a.configuration(11)
    assert np.array_equal(first, a.configuration(5)) and np.array_equal(first, b.configuration(5))
    assert not np.array_equal(first, a.configuration(6))
    assert not np.array_equal(first, _make(seed=8).configuration(5))
    assert not np.array_equal(_make(seed=3, dynamic=False).configuration(5), _make(seed=2 ** 32 + 3, dynamic=False).configuration(5))
    assert np.abs(first - a.positions).max() > 1e-3


def test_the_stream_is_not_the_einstein_stream():
    """|g|^2 = -ln u0 here and g_x^2 + g_y^2 = -2 ln u0 in thermal.normals: with the same counter the two would agree for every
    index; counter word 3 = 1 makes them independent"""
    for seed, k in ((0, 0), (2 ** 33 + 17, 9)):
        g = phonons.normal_coordinates(seed, k, 64)
        e = thermal.normals(seed, k, 64)
        same = np.isclose(2.0 * np.abs(g) ** 2, e[:, 0] ** 2 + e[:, 1] ** 2, rtol=1e-9)
        assert not same.any()
        # ... and it is the stream the definition names
        ctr = np.zeros((64, 4), dtype=np.uint32)
        ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(64), k & 0xFFFFFFFF, k >> 32, 1
        u = thermal.uniforms(thermal.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)))
        assert np.allclose(np.abs(g) ** 2, -np.log(u[:, 0]), rtol=1e-14)
        assert np.allclose(np.angle(g * np.exp(-2j * np.pi * u[:, 1])), 0.0, atol=1e-14)


def test_draw_indices_use_all_64_bits():
    assert not np.array_equal(phonons.normal_coordinates(1, 5, 16), phonons.normal_coordinates(1, 2 ** 32 + 5, 16))
    pm = _make(dynamic=False)
    assert not np.array_equal(pm.configuration(5), pm.configuration(2 ** 32 + 5))
    # a dynamic record draws once: every frame has the coefficients of frame 0 up to its phase
    C = phonons.mode_coefficients(_make().tau, 7, [0, 3], dynamic=True)
    assert np.allclose(np.abs(C[0]), np.abs(C[1]), rtol=1e-15) and not np.allclose(C[0], C[1])
    S = phonons.mode_coefficients(_make().tau, 7, [0, 3], dynamic=False)
    assert np.array_equal(S[0], C[0]) and not np.allclose(np.abs(S[1]), np.abs(S[0]))


def test_dynamic_record_is_periodic():
    """every tau_m * T an integer (tau = j / 16, T = 16): frame c + T is frame c within 4 * 2^-52 * sum_m |g_m| max_alpha |W[m, b_i, alpha]|
    per atom (frac() of the two phases may differ by roundings of tau * c only, which are exact here)"""
    pm = _make(n_frames=16)
    assert np.array_equal(pm.tau * 16, np.rint(pm.tau * 16))
    g = np.abs(phonons.normal_coordinates(pm.seed, 0, pm.n_modes))
    bound = 4 * EPS * (g[:, None] * np.abs(pm.displacements).max(axis=2)).sum(axis=0)[pm.basis_index]
    worst = 0.0
    for c in (0, 1, 7, 15, 100):
        d = np.abs(pm.configuration(c + 16) - pm.configuration(c)).max(axis=1)
        worst = max(worst, (d / bound).max())
        assert (d <= bound).all()
    assert not np.allclose(pm.configuration(0), pm.configuration(8), atol=1e-4)
    print(f"periodicity: worst |frame c+T - frame c| / bound = {worst:.3f}")


def test_snapshots_reproduce_the_variance_identity():
    """<u^2> = 1/2 sum_m |W|^2 over 4096 snapshots, five standard errors.  u = sum_m Re[g_m a_m], a_m = E W of modulus |W|; Re[g a] has
    variance v_m = |a|^2 / 2 and fourth moment |a|^4 <|g|^4> <cos^4> = |a|^4 * 2 * 3/8 = 3 v_m^2; the modes are independent with mean
    zero, so <u^4> = sum_m 3 v_m^2 + 3 (v^2 - sum_m v_m^2) = 3 v^2, var(u^2) = 2 v^2 and the standard error of the mean of N values of
    u^2 is v sqrt(2 / N)."""
    N = 4096
    pm = _make(dynamic=False, seed=11)
    C = phonons.mode_coefficients(pm.tau, pm.seed, range(N), dynamic=False)
    u = np.stack([phonons.displacements_of(pm.positions, pm.basis_index, pm.wavevectors, pm.displacements, C[c]) for c in range(N)])
    assert np.array_equal(pm.positions + u[9], pm.configuration(9))
    vm = 0.5 * np.abs(pm.displacements) ** 2                                  # (M, nb, 3)
    v = vm.sum(axis=0)
    mu4 = 3.0 * (vm ** 2).sum(axis=0) + 3.0 * (v ** 2 - (vm ** 2).sum(axis=0))
    se = np.sqrt((mu4 - v ** 2) / N)
    assert np.allclose(se, v * np.sqrt(2.0 / N), rtol=1e-12)
    assert np.allclose(pm.mean_square_displacement(), v[pm.basis_index], rtol=1e-15)
    dev = np.abs((u ** 2).mean(axis=0) - v[pm.basis_index]) / se[pm.basis_index]
    print(f"variance identity: worst deviation {dev.max():.2f} standard errors over {dev.size} components")
    assert dev.max() <= 5.0
    assert np.abs(u.mean(axis=0)).max() <= 5.0 * np.sqrt(v.max() / N)


# ---- from_eigenvectors -------------------------------------------------------------------------------------
def _eig(statistics, T_K, nu_THz=(1.0, 2.5), masses=(28.0855, 15.999), n_cells=12, **kw):
    Z, pos, box, b = _structure()
    q = np.array([[1, 0, 0], [0, 1, 0]]) / np.diag(box)
    e = np.array([[[0.6, 0, 0], [0.8, 0, 0]], [[0, 0.8j, 0], [0, 0.6, 0]]])
    return PhononModes.from_eigenvectors(Z, pos, box, b, q, e, np.asarray(masses), np.asarray(nu_THz), T_K, n_cells, 4,
                                         statistics=statistics, **kw)


def test_from_eigenvectors_amplitudes():
    """the classical amplitude against its formula in SI by hand; quantum / classical = sqrt(x coth x), x = h nu / 2 k_B T.
    coth x = 1/x + x/3 - x^3/45 + ... alternates for small x, so 1 + x^2/3 - x^4/45 <= x coth x <= 1 + x^2/3.  Tested at nu = 1 and
    2.5 THz, T = 3000 K: k_B T / h nu = 62.5 and 25, x = 8.0e-3 and 2.0e-2."""
    T = 3000.0
    cl, qu = _eig("classical", T), _eig("quantum", T)
    for m, nu in enumerate((1.0, 2.5)):
        omega = 2 * np.pi * nu * 1e12
        s = np.sqrt(2 * 1.380649e-23 * T / (omega ** 2 * 12) / 1.66053906660e-27) * 1e10
        want = s * np.array([[[0.6, 0, 0], [0.8, 0, 0]], [[0, 0.8j, 0], [0, 0.6, 0]]])[m] / np.sqrt([[28.0855], [15.999]])
        assert np.allclose(cl.displacements[m], want, rtol=1e-12, atol=0)
        x = 1.054571817e-34 * omega / (2 * 1.380649e-23 * T)           # hbar omega / 2 k_B T with the file's CODATA values
        assert 0.007 < x < 0.021
        nz = want != 0
        ratio2 = (np.abs(qu.displacements[m][nz]) / np.abs(cl.displacements[m][nz])) ** 2
        assert (ratio2 <= 1 + x ** 2 / 3 + 8 * EPS).all() and (ratio2 >= 1 + x ** 2 / 3 - x ** 4 / 45 - 8 * EPS).all()
        assert (ratio2 > 1 + 0.9 * x ** 2 / 3).all()
    assert np.array_equal(cl.frequencies, [1.0, 2.5])
    # zero-point motion: at T = 0 the quantum amplitude is hbar / omega, the classical one is refused
    z = _eig("quantum", 0.0)
    assert np.allclose(np.abs(z.displacements[0, 0, 0]),
                       np.sqrt(1.054571817e-34 / (2 * np.pi * 1e12) / 12 / 1.66053906660e-27) * 1e10 * 0.6 / np.sqrt(28.0855), rtol=1e-12)
    with pytest.raises(ValueError, match="temperature_K"):
        _eig("classical", 0.0)


def test_from_eigenvectors_scalings_and_refusals():
    base = _eig("quantum", 300.0)
    heavy = _eig("quantum", 300.0, masses=(4 * 28.0855, 15.999))
    assert np.allclose(heavy.displacements[:, 0], base.displacements[:, 0] / 2, rtol=1e-15)
    assert np.array_equal(heavy.displacements[:, 1], base.displacements[:, 1])
    big = _eig("quantum", 300.0, n_cells=48)
    assert np.allclose(big.displacements, base.displacements / 2, rtol=1e-15)
    with pytest.raises(ValueError, match="frequency 0"):
        _eig("quantum", 300.0, nu_THz=(1.0, 0.0))
    with pytest.raises(ValueError, match="statistics"):
        _eig("bose", 300.0)
    with pytest.raises(ValueError, match="masses_amu"):
        _eig("quantum", 300.0, masses=(28.0, 0.0))
    with pytest.raises(ValueError, match="n_cells"):
        _eig("quantum", 300.0, n_cells=0)


# ---- a travelling wave is a travelling wave ----------------------------------------------------------------
def test_travelling_wave_in_the_tacaw_spectrum():
    """Simple cubic, one atom per cell, a = 2 A, 4 x 4 x 2 cells in an 8 x 8 x 4 A box: a 32 x 32 grid of 0.25 A pixels, 2 slices, plane
    wave.  One longitudinal mode q = (1/Lx, 0, 0), tau = 3/16, T = 16 frames.  k_max = 1 / (2 * 0.25 A) = 2 / A, and |W| is set so
    that 2 pi k_max |g| |W| = 0.1 exactly: the displacement enters the exit wave to first order as exp(+-2 pi i (q.r - nu t)), so the
    non-zero-frequency intensity lies in the bins -+3; the second order (bins -+6) is down by (0.1 / 2)^2 at most.  The oracle gives
    0.999 of it in the bins +-3 (the condition: >= 0.9).  With the transforms of TACAWData (numpy.fft in time and space) the wave
    exp(2 pi i (q.r - nu t)) sits at frequency -nu and at G + q, its conjugate at +nu and G - q: the Bragg spots G are every fourth
    pixel, q is one pixel."""
    a, T = 2.0, 16
    box = np.diag([8.0, 8.0, 4.0])
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3) * a
    pos = cells + np.array([0.5, 0.5, 1.0])
    Z = np.full(len(pos), 14)
    seed = 3
    g = abs(phonons.normal_coordinates(seed, 0, 1)[0])
    k_max = 2.0
    w = 0.1 / (2 * np.pi * k_max * g)
    pm = PhononModes(Z, pos, box, np.zeros(len(pos), dtype=int), [[1 / 8.0, 0, 0]], [3 / 16], np.array([[[w, 0, 0]]]), T, seed=seed)
    assert 2 * np.pi * k_max * g * w <= 0.1 * (1 + 4 * EPS)
    tr = pm.to_trajectory()
    out = orc.run_frames(box, tr.positions, Z, 0.0, EV, sampling=0.255, slice_thickness=2.1)
    wf = out["wavefunction_data"]
    assert wf.shape == (1, T, 32, 32, 1) and len(out["zs"]) == 2
    assert np.isclose(out["xs"][1] - out["xs"][0], 0.25)
    freqs, I = orc.tacaw(wf, np.arange(T) * pm.timestep)
    bins = np.rint(freqs * T).astype(int)
    per_bin = I[0].sum(axis=(1, 2))
    nonzero = per_bin[bins != 0].sum()
    share = (per_bin[bins == 3].sum() + per_bin[bins == -3].sum()) / nonzero
    print(f"travelling wave: {share:.6f} of the non-zero-frequency intensity in the bins +-3")
    assert nonzero > 0 and share >= 0.9
    side = (np.arange(32) - 16) % 4                                 # kx pixel relative to the nearest Bragg row below it
    for f, own, other in ((-3, 1, 3), (3, 3, 1)):
        row = I[0][bins == f][0].sum(axis=1)                        # over ky
        assert row[side == own].sum() >= 0.99 * row.sum() and row[side == other].sum() <= 0.01 * row.sum(), f
    assert np.isclose(per_bin[bins == 3].sum(), per_bin[bins == -3].sum(), rtol=0.2)


# ---- the calculator ----------------------------------------------------------------------------------------
PP = [(1.3, 2.05), (4.8, 0.4), (0.0, 0.0), (2.5, 2.5)]
SEED = 2 ** 33 + 17


@pytest.fixture(scope="module")
def modes():
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 6, 1, ny=80, density=0.05, seed=4, species=(79, 6))
    n = tr.positions.shape[1]
    rng = np.random.default_rng(2)
    M, nb = 5, 3
    q = rng.integers(-3, 4, (M, 3)) / np.diag(tr.box_matrix)
    W = (rng.standard_normal((M, nb, 3)) + 1j * rng.standard_normal((M, nb, 3))) * 0.01
    return PhononModes(np.array([79, 6])[np.arange(n) % 2], tr.positions[0], tr.box_matrix, np.arange(n) % nb, q,
                       rng.random(M), W, 5, seed=SEED, timestep=0.25)


def _calc(**kw):
    import pyslice_amd as ps
    return ps.MultisliceCalculator(device=0, progress=False, **kw)


def _recorded(monkeypatch, source, run, **kw):
    from pyslice_amd import _native
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    calc = _calc(**kw)
    calc.setup(source, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    getattr(calc, run)()
    return calc._engine.calls


def _run_modes():
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.stem_data import Detector
    return [("run", {}),
            ("run_detectors", dict(detectors=[Detector("adf", inner=40.0, outer=120.0)], probe_batch=2)),
            ("run_diffraction", dict(diffraction=Diffraction(bin=(2, 2), split=True), probe_batch=2))]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_calculator_builds_by_index(modes, monkeypatch, mode):
    """5 frames at frame_batch = 2 (two probe batches in the probe-batch modes): one set_structure, one set_modes behind it, and
    build_modes with exactly the (first, n) sequence build_potentials gets for the 5-frame Trajectory of the same frames; everything
    else the engine is asked to do is the same, call for call"""
    run, kw = _run_modes()[mode]
    tr = modes.to_trajectory()
    got = _recorded(monkeypatch, modes, run, frame_batch=2, **kw)
    ref = _recorded(monkeypatch, tr, run, frame_batch=2, **kw)
    names = [c[0] for c in got]
    assert names.count("set_structure") == 1 and names.count("set_modes") == 1
    assert names.index("set_modes") == names.index("set_structure") + 1
    pos, Z, sigma, axis = got[names.index("set_structure")][1]
    assert np.array_equal(pos, modes.positions) and axis == 2 and not np.any(sigma) and sigma.shape == (modes.n_atoms,)
    assert Z.dtype == np.int32 and set(Z.tolist()) == {79, 6}
    b, q, tau, W, dynamic = got[names.index("set_modes")][1]
    assert np.array_equal(b, modes.basis_index) and np.array_equal(q, modes.wavevectors) and np.array_equal(W, modes.displacements)
    assert np.array_equal(tau, modes.frequencies * 0.25) and dynamic is True
    assert not [c for c in got if c[0] in ("build_potential", "build_potentials", "build_thermal")]
    calls = [c[1] for c in got if c[0] == "build_modes"]
    assert all(a[0] == SEED for a in calls)

    def first_frame(block):
        hits = [s for s in range(5) if np.array_equal(tr.positions[s:s + len(block)], block)]
        assert len(hits) == 1
        return hits[0]
    want = [(first_frame(c[1][0]), len(c[1][0])) for c in ref if c[0] == "build_potentials"]
    assert len(want) >= 3 and [(a[1], a[2]) for a in calls] == want
    if run == "run_diffraction":
        assert want == 2 * [(0, 2), (2, 2), (4, 1)]             # once per probe batch: a regeneration by index
    own = ("set_structure", "set_modes", "build_modes", "build_potentials")
    assert [c[0] for c in got if c[0] not in own] == [c[0] for c in ref if c[0] not in own]
    where = lambda calls, name: [i for i, c in enumerate(calls) if c[0] == name]
    assert [i - 2 for i in where(got, "build_modes")] == where(ref, "build_potentials")     # (the two set-up calls come earlier)


def test_prism_loop_builds_by_index_at_frame_batch_one(modes, monkeypatch):
    from pyslice_amd.prism import Prism
    from pyslice_amd.stem_data import Detector
    kw = dict(detectors=[Detector("adf", inner=40.0, outer=120.0)], probe_batch=2, prism=Prism(1))
    got = _recorded(monkeypatch, modes, "run_detectors", **kw)
    assert [c[1] for c in got if c[0] == "build_modes"] == [(SEED, s, 1) for s in range(5)]
    assert [c[0] for c in got if c[0] in ("build_modes", "smatrix_build")] == 5 * ["build_modes", "smatrix_build"]
    assert not [c for c in got if c[0] in ("build_potential", "build_potentials", "build_thermal")]


def test_other_sources_are_unchanged(modes, monkeypatch):
    """a Trajectory never reaches the new calls, and a FrozenPhonons never reaches set_modes / build_modes"""
    tr = modes.to_trajectory()
    for fb, name in ((1, "build_potential"), (2, "build_potentials")):
        calls = _recorded(monkeypatch, tr, "run", frame_batch=fb)
        assert not [c for c in calls if c[0] in ("set_structure", "set_modes", "build_modes", "build_thermal")]
        assert len([c for c in calls if c[0] == name]) == (5 if fb == 1 else 3)
    fp = thermal.FrozenPhonons(modes.atom_types, modes.positions, modes.box_matrix, 0.05, 5, seed=SEED)
    calls = _recorded(monkeypatch, fp, "run", frame_batch=2)
    assert not [c for c in calls if c[0] in ("set_modes", "build_modes")]
    assert [c[1] for c in calls if c[0] == "build_thermal"] == [(SEED, 0, 2), (SEED, 2, 2), (SEED, 4, 1)]


def test_refusals_name_phonon_modes(modes, monkeypatch, tmp_path):
    from pyslice_amd import _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(_native, "Engine", no_engine)
    monkeypatch.chdir(tmp_path)
    for kw in (dict(cache=True), dict(stream_tile=2)):
        with pytest.raises(NotImplementedError, match=r"phonon modes: .* is not built"):
            _calc(**kw).setup(modes, aperture=30.0, voltage_eV=EV, probe_positions=PP)
    assert not os.path.exists(tmp_path / "psi_data")           # refused before the cache directory is made
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r"phonon modes: .* is not built"):
        _calc().setup(modes, aperture=30.0, voltage_eV=EV, probe_positions=PP)


def test_entry_points_in_the_binding_and_library():
    from pyslice_amd import build_native, _native
    build_native.build()
    lib = _native.load()
    for name in ("msl_set_modes", "msl_build_modes", "msl_mode_positions"):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    for name in ("set_modes", "build_modes", "mode_positions"):
        assert callable(getattr(_native.Engine, name))
    assert lib.msl_build_modes(None, 0, 0, 1) == _native.MSL_ERR_INVALID
    assert lib.msl_mode_positions(None, 0, 0, None) == _native.MSL_ERR_INVALID
    assert lib.msl_set_modes(None, None, 0, 1, None, None, None, 1, 1) == _native.MSL_ERR_INVALID
