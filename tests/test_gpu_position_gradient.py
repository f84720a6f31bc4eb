"""Gradients with respect to atom positions on the MI355X: msl_adjoint_positions -- Gamma to c64 images, the
handle's 2-D FFT, position_gradient_kernel on the phase tables the build left -- and run_gradient() with Gradient(positions=True),
against the float64 definition (adjoint.position_gradient) on the inputs of tests/position_gradient_cases.py.

Bounds (position_gradient_cases.py, gradient_cases.py):
  chain alone          |got - want| <= 2e-5 position_gradient_bound per atom and component, white Gamma, flat form factors
  through the run  (a) .positions against the float64 chain on the device's own .potential: the chain bound
                   (b) .positions against the full float64 definition: c ||kx f_Z||_2 sqrt N gradient_bound[s] + the chain bound
  directional          (L(r + h d) - L(r - h d)) / 2h of the device's losses against <.positions, d>: the loss bounds at the two ends
                       over 2h + twice the float64 truncation at that h + the chain bound contracted with |d| (not bound (b), which
                       would exceed <.positions, d> itself); <.positions, d> is at least 5 tolerances
  descent              the device losses of three position_step()s follow the float64 ones within loss_bound"""
import functools

import numpy as np
import pytest

import gradient_cases as gc
import position_gradient_cases as pc

pytestmark = pytest.mark.gpu

AX = (-2, -1)


def npy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def engine(case, tab, n_probes=1, **kw):
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    eng = _native.Engine(case.nx, case.ny, case.nz, case.dx, case.dy, case.dz, gc.orc.wavelength(gc.EV), gc.orc.interaction_sigma(gc.EV),
                         n_probes=n_probes, **kw)
    eng.set_kirkland(tab)
    eng.set_slices(*slice_edges(pc.slice_coords(case)))
    return eng


def calculator(ps, grid, **kw):
    calc = ps.MultisliceCalculator(device=0, progress=False, **kw)
    calc.setup(gc.trajectory(*grid), aperture=30.0, voltage_eV=gc.EV, probe_positions=gc.PP, sampling=0.1, slice_thickness=1.0)
    return calc


def gradient_calc(ps, grid, loss="amplitude", positions=True, probe_batch=2):
    c = gc.case(*grid)
    return calculator(ps, grid, gradient=ps.Gradient(loss=loss, epsilon=gc.epsilon_of(c, loss), positions=positions), probe_batch=probe_batch)


def chain(case, physical=False):
    pos, Z = pc.atoms(case)
    eng = engine(case, pc.table(case, physical))
    eng.build_potential(pos, Z, case.slice_axis)
    return eng, eng.adjoint_positions(pc.white_gamma(case))


@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_on_white_gamma(case):
    eng, got = chain(case)
    want, bound = pc.chain_reference(case)
    ratio = pc.chain_ratio(case, got)
    print(f"chain {case.name}: worst |got - want| / (2e-5 bound) {ratio:.3e}; max |want| / bound {np.abs(want[:, pc.in_plane(case)]).max() / bound.max():.3f}; "
          f"{int((bound[:, 0] == 0).sum())} atoms outside")
    assert got.shape == want.shape and got.dtype == np.float64
    assert ratio <= 1.0
    assert np.abs(want).max() > 0
    assert eng.adjoint_positions(pc.white_gamma(case)).tobytes() == got.tobytes()      # no atomics: the same bits


def test_chain_with_physical_tables():
    case = pc.PHYSICAL_CASE
    _, got = chain(case, physical=True)
    ratio = pc.chain_ratio(case, got, physical=True)
    print(f"chain {case.name} physical: worst |got - want| / (2e-5 bound) {ratio:.3e}")
    assert ratio <= 1.0


@functools.lru_cache(maxsize=None)
def device_run(grid, loss):
    import pyslice_amd
    return gradient_calc(pyslice_amd, grid, loss=loss).run_gradient(gc.case(*grid)["D"])


@pytest.mark.parametrize("grid", pc.RUN_GRIDS)
@pytest.mark.parametrize("loss", gc.LOSSES)
def test_through_the_run(ps, grid, loss):
    from pyslice_amd.adjoint import position_gradient, position_gradient_bound
    res = device_run(grid, loss)
    tr = gc.trajectory(*grid)
    xs, ys, zs = pc.run_axes(grid)
    pos, Z = tr.positions[0], tr.atom_types
    assert res.positions.shape == (len(Z), 3) and res.positions.dtype == np.float64 and not res.positions[:, 2].any()
    gam = np.moveaxis(res.potential, 2, 0)
    want_a, bound_a = position_gradient(xs, ys, zs, pos, Z, gam), pc.CHAIN_TOL * position_gradient_bound(xs, ys, zs, pos, Z, gam)
    err_a = np.abs(res.positions[:, :2] - want_a[:, :2])
    ref = pc.run_reference(grid, loss)
    bound_b = pc.run_bound(grid, ref)
    err_b = np.abs(res.positions[:, :2] - ref["positions"][:, :2])
    live = ref["bound"][:, 0] > 0
    print(f"run {loss} {grid}: (a) worst / bound {(err_a[live] / bound_a[live]).max():.3e}; (b) worst / bound {(err_b[live] / bound_b[live]).max():.3e} "
          f"(max |want| / bound (b) {(np.abs(ref['positions'][live][:, :2]) / bound_b[live]).max():.3e})")
    assert (err_a <= bound_a).all()
    assert (err_b <= bound_b).all()
    assert not res.positions[~live].any() and np.abs(ref["positions"]).max() > 0


@functools.lru_cache(maxsize=None)
def directional64(grid):
    """h for the directional test, chosen in float64: the largest of a few steps at which twice the truncation |fd - <grad, d>| is
    below a tenth of the loss term of the tolerance; -> (d, h, fd64, inner64, loss_term)"""
    from pyslice_amd.adjoint import _potential_of, forward_waves, loss_and_residual, position_directional_check
    c = gc.case(*grid)
    tr = gc.trajectory(*grid)
    xs, ys, zs = pc.run_axes(grid)
    pos, Z = tr.positions[0], tr.atom_types
    d = pc.smooth_shift(len(Z))
    d[:, 2] = 0.0                                                   # (in the plane: nobody changes slice)
    for h in (0.05, 0.02, 0.01, 0.005, 0.002, 0.001):
        fd64, inner64 = position_directional_check(xs, ys, zs, pos, Z, c["probes"], c["D"], c["sigma"], c["prop"], d, h)
        loss_term = 0.0
        for sign in (+1.0, -1.0):
            Psi = forward_waves(c["probes"], _potential_of(xs, ys, zs, pos + sign * h * d, Z), c["sigma"], c["prop"])[2]
            loss_term += gc.loss_bound(c, dict(Psi=Psi, loss=loss_and_residual(Psi, c["D"])[0]), "amplitude").sum() / (2.0 * h)
        if 2.0 * abs(fd64 - inner64) <= 0.1 * loss_term:
            return d, h, fd64, inner64, loss_term
    raise AssertionError("no step found")


def test_directional_derivative_on_the_device(ps):
    grid = pc.RUN_GRIDS[0]
    tr = gc.trajectory(*grid)
    pos = tr.positions[0]
    d, h, fd64, inner64, loss_term = directional64(grid)
    calc = gradient_calc(ps, grid)
    c = gc.case(*grid)
    res = calc.run_gradient(c["D"], positions=pos)
    up = calc.run_gradient(c["D"], positions=pos + h * d).total
    down = calc.run_gradient(c["D"], positions=pos - h * d).total
    fd, inner = (up - down) / (2.0 * h), float((res.positions * d).sum())
    trunc = 2.0 * abs(fd64 - inner64)
    chain_term = float((pc.CHAIN_TOL * pc.run_reference(grid)["bound"] * np.abs(d[:, :2])).sum())
    print(f"directional {grid}: h {h}; device fd {fd:.6e} <grad, d> {inner:.6e} |diff| {abs(fd - inner):.3e}; tolerance: loss {loss_term:.3e} + "
          f"truncation {trunc:.3e} + chain {chain_term:.3e}; float64 {fd64:.6e} {inner64:.6e}")
    assert abs(fd - inner) <= loss_term + trunc + chain_term
    assert abs(inner) >= 5.0 * (loss_term + trunc + chain_term)     # (a gradient of zeros, or of the other sign, misses the tolerance)


def test_bits_override_and_batches(ps):
    grid = pc.RUN_GRIDS[1]
    c = gc.case(*grid)
    tr = gc.trajectory(*grid)
    calc = gradient_calc(ps, grid)
    r1 = calc.run_gradient(c["D"])
    r2 = calc.run_gradient(c["D"])
    over = calc.run_gradient(c["D"], positions=tr.positions[0])
    for r in (r2, over):
        assert r.positions.tobytes() == r1.positions.tobytes() and r.potential.tobytes() == r1.potential.tobytes()
        assert r.loss.tobytes() == r1.loss.tobytes()
    assert np.abs(r1.positions).max() > 0
    whole = gradient_calc(ps, grid, probe_batch=3).run_gradient(c["D"])
    diff = np.abs(whole.positions - r1.positions).max()
    print(f"probe_batch 2 against 3 {grid}: max |difference| {diff:.3e} of max |grad| {np.abs(r1.positions).max():.3e}")
    assert diff <= 1e-6 * np.abs(r1.positions).max()
    # positions=False is what it was: no .positions, and the same bits as the run that has them
    plain = gradient_calc(ps, grid, positions=False).run_gradient(c["D"])
    assert plain.positions is None and plain.potential.tobytes() == r1.potential.tobytes() and plain.loss.tobytes() == r1.loss.tobytes()
    with pytest.raises(ValueError, match="potential="):
        calc.run_gradient(c["D"], potential=np.zeros(grid))
    with pytest.raises(ValueError, match="potential="):
        gradient_calc(ps, grid, positions=False).run_gradient(c["D"], potential=np.zeros(grid), positions=tr.positions[0])
    with pytest.raises(ValueError, match="position_step"):
        plain.position_step(tr.positions[0], 1.0)


def test_other_runs_are_untouched(ps):
    grid = gc.CASES[0]
    c = gc.case(*grid)
    before = npy(calculator(ps, grid, diffraction=ps.Diffraction()).run_diffraction().intensity)
    plain_before = gradient_calc(ps, grid, positions=False).run_gradient(c["D"])
    assert gradient_calc(ps, grid).run_gradient(c["D"]).positions is not None
    after = npy(calculator(ps, grid, diffraction=ps.Diffraction()).run_diffraction().intensity)
    plain_after = gradient_calc(ps, grid, positions=False).run_gradient(c["D"])
    assert before.tobytes() == after.tobytes()
    assert plain_before.potential.tobytes() == plain_after.potential.tobytes() and plain_before.loss.tobytes() == plain_after.loss.tobytes()


def test_state_errors():
    case = pc.POW2
    pos, Z = pc.atoms(case)
    gam = pc.white_gamma(case)
    eng = engine(case, pc.table(case))
    with pytest.raises(RuntimeError, match="msl_build_potential"):
        eng.adjoint_positions(gam)                                  # no build at all
    eng.build_potential(pos, Z)
    got = eng.adjoint_positions(gam)
    with pytest.raises(RuntimeError, match="msl_set_adjoint"):
        eng.adjoint_positions()                                     # no accumulator
    # the exit waves of a slice loop are not touched by the chain
    eng.set_probes(30.0, np.asarray([(1.6, 1.6)]))
    eng.propagate()
    own = eng.exit_waves()
    assert eng.adjoint_positions(gam).tobytes() == got.tobytes()
    assert eng.exit_waves().tobytes() == own.tobytes()
    eng.upload_potential(np.zeros((case.nz, case.nx, case.ny), dtype=np.float32))
    with pytest.raises(RuntimeError, match="msl_build_potential"):
        eng.adjoint_positions(gam)
    eng.build_potential(pos, Z)
    assert eng.adjoint_positions(gam).tobytes() == got.tobytes()
    eng.set_projection(1, 2)
    with pytest.raises(RuntimeError, match="msl_build_potential"):
        eng.adjoint_positions(gam)
    assert eng._lib.msl_adjoint_positions_rows(eng._h) == -1
    limited = engine(case, pc.table(case))
    limited.set_bandlimit(8, 6)
    limited.build_potential(pos, Z)
    with pytest.raises(RuntimeError, match="msl_build_potential"):
        limited.adjoint_positions(gam)                              # (V is low-passed behind the structure factor)
    batched = engine(case, pc.table(case), n_frames=2, frame_batch=2)
    batched.build_potentials(np.stack([pos, pos]), Z)
    with pytest.raises(RuntimeError, match="msl_build_potential"):
        batched.adjoint_positions(gam)
    # the accumulator as Gamma, and the timing entry
    acc = engine(case, pc.table(case, True))
    acc.build_potential(pos, Z)
    acc.set_probes(30.0, np.asarray([(1.6, 1.6)]))
    acc.set_adjoint(1, 1e-20, None)
    acc.adjoint_add(np.ones((1, case.nx, case.ny), dtype=np.float32), 1)
    from_acc = acc.adjoint_positions()
    assert from_acc.tobytes() == acc.adjoint_positions(acc.adjoint_download()).tobytes() and np.abs(from_acc).max() > 0
    assert acc.adjoint_positions_time(2) > 0.0
    assert acc.adjoint_positions().tobytes() == from_acc.tobytes()


@functools.lru_cache(maxsize=None)
def descent64(grid):
    """three position_step()s on the amplitude loss against the patterns of the true structure, from atoms displaced by a seeded
    0.03 A Gaussian, in float64: the rate -- the largest L / ||grad||^2 / 2^k at which the loss falls at every step -- and per step
    the loss and its bound"""
    from pyslice_amd.adjoint import _potential_of, forward_waves, position_gradient, potential_gradient
    c = gc.case(*grid)
    tr = gc.trajectory(*grid)
    xs, ys, zs = pc.run_axes(grid)
    pos0, Z = tr.positions[0], tr.atom_types
    data = np.fft.fftshift(np.abs(forward_waves(c["probes"], _potential_of(xs, ys, zs, pos0, Z), c["sigma"], c["prop"])[2]) ** 2, axes=AX)
    start = pos0 + 0.03 * np.random.default_rng(21).standard_normal(pos0.shape)

    def run(rate):
        pos, out = start.copy(), []
        for _ in range(4):
            grad, L, _, det = potential_gradient(c["probes"], _potential_of(xs, ys, zs, pos, Z), data, c["sigma"], c["prop"], details=True)
            g = position_gradient(xs, ys, zs, pos, Z, grad)
            out.append((L.sum(), gc.loss_bound(c, dict(Psi=det["Psi"], loss=L), "amplitude").sum(), g))
            pos = pos - rate * g
        return out
    first = run(0.0)[0]
    rate = first[0] / (first[2] ** 2).sum()
    for _ in range(30):
        steps = run(rate)
        if all(steps[k + 1][0] < steps[k][0] for k in range(3)):
            return data, start, rate, [(s[0], s[1]) for s in steps]
        rate /= 2.0
    raise AssertionError("no rate found")


def test_three_position_steps_follow_the_float64_sequence(ps):
    grid = pc.RUN_GRIDS[0]
    data, pos, rate, want = descent64(grid)
    calc = gradient_calc(ps, grid)
    got = []
    for k in range(4):
        res = calc.run_gradient(data, positions=pos)
        got.append(res.total)
        pos = res.position_step(pos, rate)
    print(f"position descent {grid}: rate {rate:.4e}; device {got}; float64 {[w[0] for w in want]}; bounds {[w[1] for w in want]}")
    for k in range(4):
        assert abs(got[k] - want[k][0]) <= want[k][1], k
    assert got[3] < got[2] < got[1] < got[0]
