"""Gradients on the MI355X: run_gradient() -- the forward loop with the store, the residual pass, the backward loop -- against the
float64 definition (pyslice_amd/adjoint.py) on the inputs of tests/gradient_cases.py: Si + O cells, 0.1 A pixels, 1 A slices,
100 kV; 256 x 64 and 64 x 256 (the fast row kernel), 96 x 80 (generic lines), 101 x 97 (the odd pitch tail and the odd-length shift
mapping); nz = 1 (no propagator), 2 and 4; 3 probes at probe_batch=2 (a full and a ragged batch, accumulated).  The potential is
uploaded (potential=), so the device and the definition start from the same float32 numbers; D are the patterns of 0.9 V.

Bounds, with eps = 1e-4 the rel-L2 the parity tests allow the waves (gradient_cases.py):
  gradient, per slice   ||got_s - want_s||_1 <= 3 eps 2 sigma sum_p ||g_p,s||_2 ||phi_p,s||_2   (gradient_bound)
  loss, per probe       amplitude 2 eps sqrt(L S) + eps^2 S, S = sum I; intensity and Poisson: the docstring of loss_bound
  probe gradient        rel-L2 <= 3 eps
  directional           (L(V + h d) - L(V - h d)) / 2h against <grad, d> at h = 5 (d of unit maximum, V up to 3e3): the two loss
                        bounds, at V + h d and at V - h d, over 2h (4.9e-4 at 96 x 80 x 4) + twice the float64 truncation at that h (3.6e-7) + the gradient bound
                        contracted with d (at most sum_s bound_s, 2.7e-5); <grad, d> = 1.87e-3."""
import functools

import numpy as np
import pytest

import gradient_cases as gc

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


def calculator(ps, grid, **kw):
    calc = ps.MultisliceCalculator(device=0, progress=False, **kw)
    calc.setup(gc.trajectory(*grid), aperture=30.0, voltage_eV=gc.EV, probe_positions=gc.PP, sampling=0.1, slice_thickness=1.0)
    return calc


def gradient_calc(ps, grid, loss="amplitude", weighted=False, probe=False, probe_batch=2):
    c = gc.case(*grid)
    g = ps.Gradient(loss=loss, weight=gc.disc_weight(grid[0], grid[1]) if weighted else None, epsilon=gc.epsilon_of(c, loss), probe=probe)
    return calculator(ps, grid, gradient=g, probe_batch=probe_batch)


def nxnynz(V):
    return np.ascontiguousarray(np.moveaxis(V, 0, 2))


def check(tag, res, c, ref, loss):
    """the gradient and loss bounds of the module; prints every figure before it asserts"""
    got = np.moveaxis(res.potential, 2, 0)
    err, bound = np.abs(got - ref["grad"]).sum(axis=AX), gc.gradient_bound(c, ref)
    lerr, lbound = np.abs(res.loss - ref["loss"]), gc.loss_bound(c, ref, loss)
    print(f"{tag}: gradient worst ||got - want||_1 / bound {(err / bound).max():.3e} (of ||want||_1 {(err / np.abs(ref['grad']).sum(axis=AX)).max():.3e}); "
          f"loss worst |got - want| / bound {(lerr / lbound).max():.3e} (L {ref['loss'].max():.3e})")
    assert (err <= bound).all(), (err / bound)
    assert (lerr <= lbound).all(), (lerr / lbound)
    assert np.abs(ref["grad"]).max() > 0


@pytest.mark.parametrize("grid", gc.CASES)
def test_gradient_loss_and_probe_gradient(ps, grid):
    c, ref = gc.case(*grid), gc.reference(*grid)
    res = gradient_calc(ps, grid, probe=True).run_gradient(c["D"], potential=nxnynz(c["V"]))
    assert res.potential.shape == grid and res.potential.dtype == np.float64 and res.loss.shape == (3,)
    check(f"gradient {grid}", res, c, ref, "amplitude")
    perr = np.sqrt((np.abs(res.probe - ref["probe"]) ** 2).sum(axis=AX) / (np.abs(ref["probe"]) ** 2).sum(axis=AX))
    print(f"gradient {grid}: probe gradient rel-L2 per probe {perr} (3e-4)")
    assert (perr <= 3.0 * gc.EPS).all()
    assert abs(res.total - ref["loss"].sum()) <= gc.loss_bound(c, ref, "amplitude").sum()


@pytest.mark.parametrize("grid", [gc.CASES[3], gc.CASES[4]])
@pytest.mark.parametrize("loss", ["intensity", "poisson"])
def test_other_losses(ps, grid, loss):
    c, ref = gc.case(*grid), gc.reference(*grid, loss=loss)
    res = gradient_calc(ps, grid, loss=loss).run_gradient(c["D"], potential=nxnynz(c["V"]))
    check(f"gradient {loss} {grid}", res, c, ref, loss)
    assert res.probe is None and res.kind == loss


@pytest.mark.parametrize("grid", [gc.CASES[1], gc.CASES[4]])
def test_weight_zero_outside_a_disc(ps, grid):
    c, ref = gc.case(*grid), gc.reference(*grid, weighted=True)
    res = gradient_calc(ps, grid, weighted=True).run_gradient(c["D"], potential=nxnynz(c["V"]))
    check(f"gradient weighted {grid}", res, c, ref, "amplitude")
    plain = gc.reference(*grid)
    assert np.abs(ref["grad"] - plain["grad"]).sum() > 100.0 * gc.gradient_bound(c, plain).sum()     # (the weight is seen)


def test_directional_derivative_on_the_device(ps):
    """h and the three terms of the tolerance: the module's docstring"""
    from pyslice_amd.adjoint import directional_check
    grid = gc.CASES[3]
    c, ref = gc.case(*grid), gc.reference(*grid)
    d, h = gc.smooth_direction(*grid), gc.DIRECTION_H
    calc = gradient_calc(ps, grid)
    res = calc.run_gradient(c["D"], potential=nxnynz(c["V"]))
    up = calc.run_gradient(c["D"], potential=nxnynz(c["V"] + h * d)).total
    down = calc.run_gradient(c["D"], potential=nxnynz(c["V"] - h * d)).total
    fd, inner = (up - down) / (2.0 * h), float((np.moveaxis(res.potential, 2, 0) * d).sum())
    fd64, inner64 = directional_check(c["probes"], c["V"], c["D"], c["sigma"], c["prop"], d, h)
    from pyslice_amd.adjoint import forward_waves, loss_and_residual
    loss_term = 0.0                                                 # the loss bounds at V + h d and at V - h d, over 2h
    for sign in (+1.0, -1.0):
        Vs = (c["V"] + sign * h * d).astype(np.float32).astype(np.float64)
        Psi = forward_waves(c["probes"], Vs, c["sigma"], c["prop"])[2]
        loss_term += gc.loss_bound(c, dict(Psi=Psi, loss=loss_and_residual(Psi, c["D"])[0]), "amplitude").sum() / (2.0 * h)
    trunc, grad_term = 2.0 * abs(fd64 - inner64), float((gc.gradient_bound(c, ref)[:, None, None] * np.abs(d)).max(axis=AX).sum())
    print(f"directional {grid}: device fd {fd:.6e} <grad, d> {inner:.6e} |diff| {abs(fd - inner):.3e}; tolerance: loss {loss_term:.3e} + "
          f"truncation {trunc:.3e} + gradient {grad_term:.3e}; float64 {fd64:.6e} {inner64:.6e}")
    assert abs(fd - inner) <= loss_term + trunc + grad_term


def test_bits_and_reset(ps):
    """two run_gradient() calls give the same bits; the second -- a reset behind an add -- equals the first of a fresh handle; and the
    built frame (no potential=) runs the same path"""
    grid = gc.CASES[4]
    c = gc.case(*grid)
    a = gradient_calc(ps, grid, probe=True)
    r1 = a.run_gradient(c["D"])
    r2 = a.run_gradient(c["D"], frame=0)
    fresh = gradient_calc(ps, grid, probe=True).run_gradient(c["D"])
    for r in (r2, fresh):
        assert r.potential.tobytes() == r1.potential.tobytes() and r.loss.tobytes() == r1.loss.tobytes()
        assert r.probe.tobytes() == r1.probe.tobytes()
    assert np.abs(r1.potential).max() > 0
    # another probe batch: the float64 sums over the probes in another order, and nothing else
    whole = gradient_calc(ps, grid, probe_batch=3).run_gradient(c["D"])
    assert whole.loss.tobytes() == r1.loss.tobytes()
    diff = np.abs(whole.potential - r1.potential).max()
    print(f"probe_batch 2 against 3 {grid}: max |difference| {diff:.3e} of max |grad| {np.abs(r1.potential).max():.3e}")
    assert diff <= 1e-6 * np.abs(r1.potential).max()


def test_own_patterns_give_no_loss(ps):
    grid = gc.CASES[3]
    c = gc.case(*grid)
    data = calculator(ps, grid, diffraction=ps.Diffraction(), probe_batch=2).run_diffraction()
    res = gradient_calc(ps, grid).run_gradient(data)
    S = npy(data.intensity).sum(axis=AX)
    bound = gc.EPS ** 2 * S                                         # (the amplitude bound at L = 0)
    print(f"own patterns {grid}: loss {res.loss} bound {bound}")
    assert (res.loss <= bound).all() and (res.loss >= 0).all()


def test_handle_state(ps):
    """a plain run_diffraction() is the same bit for bit before and after a gradient run in the process, and msl_set_adjoint(0) puts a
    handle back on its own loop"""
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    grid = gc.CASES[0]                                              # (256 x 64: planned for the one-pass loop)
    c = gc.case(*grid)
    before = npy(calculator(ps, grid, diffraction=ps.Diffraction()).run_diffraction().intensity)
    gradient_calc(ps, grid).run_gradient(c["D"])
    after = npy(calculator(ps, grid, diffraction=ps.Diffraction()).run_diffraction().intensity)
    assert before.tobytes() == after.tobytes()
    xs, ys, zs = c["xs"], c["ys"], c["zs"]
    eng = _native.Engine(grid[0], grid[1], grid[2], xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], gc.orc.wavelength(gc.EV), c["sigma"], n_probes=3)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(zs))
    eng.upload_potential(c["V"])
    eng.set_probes(30.0, np.asarray(gc.PP))
    eng.propagate()
    own = eng.exit_waves()
    eng.set_adjoint(1, 1e-20, None)
    loss, _ = eng.adjoint_add(c["D"], 3)
    g1 = eng.adjoint_download()
    eng.adjoint_reset()
    assert not eng.adjoint_download().any()
    eng.adjoint_add(c["D"], 3)
    assert eng.adjoint_download().tobytes() == g1.tobytes()
    # the timing entry runs the step alone; a reset behind it and the next add give the same bits again
    assert eng.adjoint_step_time(grid[2] - 1, 2) > 0.0
    eng.adjoint_reset()
    eng.adjoint_add(c["D"], 3)
    assert eng.adjoint_download().tobytes() == g1.tobytes()
    eng.set_adjoint(0)
    eng.propagate()
    assert eng.exit_waves().tobytes() == own.tobytes()
    with pytest.raises(RuntimeError):
        eng.adjoint_add(c["D"], 3)
    eng.set_bandlimit(20, 6)
    with pytest.raises(NotImplementedError):
        eng.set_adjoint(1, 1e-20, None)


@functools.lru_cache(maxsize=None)
def descent64(grid):
    """three steps of plain descent on the amplitude loss against the patterns of V, from 0.9 V, in float64: the rate -- the largest
    L / ||grad||^2 / 2^k at which the loss falls at every step -- and per step the loss and its bound"""
    from pyslice_amd.adjoint import forward_waves, potential_gradient
    c = gc.case(*grid)
    data = np.fft.fftshift(np.abs(forward_waves(c["probes"], c["V"], c["sigma"], c["prop"])[2]) ** 2, axes=AX)

    def run(rate):
        V, out = c["V09"].copy(), []
        for _ in range(4):
            V32 = V.astype(np.float32).astype(np.float64)
            grad, L, _, det = potential_gradient(c["probes"], V32, data, c["sigma"], c["prop"], details=True)
            out.append((L.sum(), gc.loss_bound(c, dict(Psi=det["Psi"], loss=L), "amplitude").sum(), grad))
            V = V - rate * grad
        return out
    first = run(0.0)[0]
    rate = first[0] / (first[2] ** 2).sum()
    for _ in range(20):
        steps = run(rate)
        if all(steps[k + 1][0] < steps[k][0] for k in range(3)):
            return data, rate, [(s[0], s[1]) for s in steps]
        rate /= 2.0
    raise AssertionError("no rate found")


def test_three_descent_steps_follow_the_float64_sequence(ps):
    grid = gc.CASES[3]
    c = gc.case(*grid)
    data, rate, want = descent64(grid)
    calc = gradient_calc(ps, grid)
    V = nxnynz(c["V09"])
    got = []
    for k in range(4):
        res = calc.run_gradient(data, potential=V)
        got.append(res.total)
        V = res.descent_step(V, rate)
    print(f"descent {grid}: rate {rate:.4e}; device {got}; float64 {[w[0] for w in want]}; bounds {[w[1] for w in want]}")
    for k in range(4):
        assert abs(got[k] - want[k][0]) <= want[k][1], k
    assert got[3] < got[2] < got[1] < got[0]
