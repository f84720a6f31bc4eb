"""Gradients with respect to scan positions and probe aberrations on the MI355X: msl_adjoint_probe_params --
the handle's 2-D FFT of the probe gradient and probe_moment_kernel over the aperture's box -- and run_gradient() with
Gradient(probe_positions=True, aberrations=True), against the float64 definition (adjoint.probe_parameter_gradient) on the inputs of
tests/probe_gradient_cases.py.

Bounds (probe_gradient_cases.py):
  chain alone          |got - want| <= (4 pi / N) ||b A||_2 tol ||ghat_p||_2 + 1e-12 sum |b| |ghat_p| per probe and parameter, white g0
  through the run  (a) the results against the float64 chain on the device's own probe gradient: the chain bound
                   (b) against the full float64 definition: (4 pi / N) ||b A||_2 sqrt N 3e-4 ||g0_p||_2 + the chain bound
  directional          (L(+h d) - L(-h d)) / 2h of the device's losses through run_gradient(probe_positions=, aberrations=) against
                       <grad, d>, d mixing every scan position with defocus, astigmatism and Cs at a non-zero lens: the loss bounds at
                       the two ends over 2h + twice the float64 truncation at that h + the chain bound contracted with |d|;
                       <grad, d> is at least 5 tolerances
  probe_batch 2 | 3    equal losses, results within the chain bound of each other
  descent              the device losses of three probe_position_step()s and of three aberration_step()s follow the float64 ones
                       within loss_bound, and fall"""
import functools

import numpy as np
import pytest

import gradient_cases as gc
import probe_gradient_cases as pc

pytestmark = pytest.mark.gpu


def npy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def engine(nx, ny, n_probes, nz=1):
    from pyslice_amd import _native
    return _native.Engine(nx, ny, nz, pc.DX, pc.DX, 1.0, pc.wavelength(), gc.orc.interaction_sigma(gc.EV), n_probes=n_probes)


# ---- 1. the chain alone ----
@pytest.mark.parametrize("aberrated", [True, False], ids=["aberrated", "zero"])
@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_on_white_g0(case, aberrated):
    want, bound = pc.chain_reference(case, aberrated)
    g0 = pc.white_g0(case)
    eng = engine(case.nx, case.ny, 3)
    eng.set_aberrations(pc.aberr() if aberrated else None)
    eng.set_probes(case.mrad, pc.PP)
    got = eng.adjoint_probe_params(g0)
    r3 = pc.ratio(got, want, bound)
    assert got.shape == (3, 30) and got.dtype == np.float64
    assert eng.adjoint_probe_params(g0).tobytes() == got.tobytes()                  # no atomics: the same bits
    two = eng.adjoint_probe_params(g0[:2])                                           # B = 2 of 3
    assert two.tobytes() == got[:2].tobytes()
    one = engine(case.nx, case.ny, 1)                                                # an engine of one probe: the last of the three
    one.set_aberrations(pc.aberr() if aberrated else None)
    one.set_probes(case.mrad, pc.PP[2:])
    r1 = pc.ratio(one.adjoint_probe_params(g0[2:]), want[2:], bound[2:])
    size = float((np.abs(want)[bound > 0] / bound[bound > 0]).max())
    print(f"chain {case.name} {'aberrated' if aberrated else 'zero'}: worst |got - want| / bound {max(r3, r1):.3e} (|want| is up to {size:.3e} bounds)")
    assert max(r3, r1) <= 1.0
    assert size >= 10.0                                                              # (a result of zeros would miss the bound)


# ---- 2. through the run ----
def calculator(ps, grid, **kw):
    calc = ps.MultisliceCalculator(device=0, progress=False, **kw)
    calc.setup(gc.trajectory(*grid), aperture=30.0, voltage_eV=gc.EV, probe_positions=gc.PP, sampling=0.1, slice_thickness=1.0)
    return calc


def gradient_calc(ps, grid, loss="amplitude", probe_batch=2, **flags):
    c = gc.case(*grid)
    return calculator(ps, grid, gradient=ps.Gradient(loss=loss, epsilon=gc.epsilon_of(c, loss), **flags), probe_batch=probe_batch)


FLAGS = dict(probe=True, probe_positions=True, aberrations=True)


@functools.lru_cache(maxsize=None)
def device_run(grid, loss, probe_batch=2):
    import pyslice_amd
    return gradient_calc(pyslice_amd, grid, loss=loss, probe_batch=probe_batch, **FLAGS).run_gradient(gc.case(*grid)["D"])


def packed(res):
    """(P, 30) of a run's results: the positions per probe; the lens terms are summed over the probes, so row 0 carries them"""
    out = np.zeros((len(res.probe_position_gradient), 30))
    out[:, :2] = res.probe_position_gradient
    out[0, 2:] = res.aberration_gradient_cartesian.reshape(28)
    return out


def summed(rows):
    out = rows.copy()
    out[0, 2:] = rows[:, 2:].sum(axis=0)
    out[1:, 2:] = 0.0
    return out


@pytest.mark.parametrize("grid", pc.RUN_GRIDS)
@pytest.mark.parametrize("loss", gc.LOSSES)
def test_through_the_run(ps, grid, loss):
    from pyslice_amd.adjoint import aberration_polar_gradient, probe_parameter_gradient
    res = device_run(grid, loss)
    got = packed(res)
    assert res.probe_position_gradient.shape == (3, 2) and res.aberration_gradient_cartesian.shape == (14, 2)
    # (a) the float64 chain on the device's own probe gradient
    g0 = res.probe.astype(np.complex128)
    pos, _, per = probe_parameter_gradient(g0, *pc.run_geometry(grid), gc.PP)
    want_a, bound_a = summed(pc.pack(pos, per)), summed(pc.chain_bound_of(g0, grid))
    ra = pc.ratio(got, want_a, bound_a)
    # (b) the full float64 definition
    ref = pc.run_reference(grid, loss)
    want_b, bound_b = summed(ref["params"]), summed(pc.run_bound_b(grid, ref["probe"]))
    rb = pc.ratio(got, want_b, bound_b)
    size = float((np.abs(want_b)[bound_b > 0] / bound_b[bound_b > 0]).max())
    print(f"run {loss} {grid}: (a) worst / bound {ra:.3e}; (b) worst / bound {rb:.3e} (|want| is up to {size:.3e} bounds (b))")
    assert ra <= 1.0
    assert rb <= 1.0
    dC, dphi = aberration_polar_gradient(res.aberration_gradient_cartesian, None, pc.wavelength())
    assert res.aberration_gradient["C10"] == dC[0] and res.aberration_gradient["C30"] == dC[4] and res.aberration_gradient["phi12"] == 0.0


# ---- 3. the directional derivative on the device ----
def uploaded(grid):
    """the potential of gradient_cases in the layout of run_gradient(potential=): the float64 model starts from the same numbers"""
    return np.ascontiguousarray(np.moveaxis(gc.case(*grid)["V"], 0, 2))


def test_directional_derivative_on_the_device(ps):
    grid = pc.RUN_GRIDS[0]
    m = pc.directional64(grid)
    h, D, V, xy = m["h"], gc.case(*grid)["D"], uploaded(grid), np.asarray(gc.PP, dtype=np.float64)
    calc = gradient_calc(ps, grid, probe_positions=True, aberrations=True)           # setup() has no lens: every run overrides it
    res = calc.run_gradient(D, potential=V, probe_positions=xy, aberrations=pc.lens0())
    up = calc.run_gradient(D, potential=V, probe_positions=xy + h * pc.D_XY, aberrations=pc.lens_at(pc.lens0(), +h)).total
    down = calc.run_gradient(D, potential=V, probe_positions=xy - h * pc.D_XY, aberrations=pc.lens_at(pc.lens0(), -h)).total
    fd = (up - down) / (2.0 * h)
    inner = float((res.probe_position_gradient * pc.D_XY).sum()) + pc.lens_inner(res.aberration_gradient)
    tol = m["loss_term"] + m["trunc"] + m["chain"]
    print(f"directional {grid}: h {h}; device fd {fd:.6e} <grad, d> {inner:.6e} |diff| {abs(fd - inner):.3e}; tolerance: loss {m['loss_term']:.3e} + "
          f"truncation {m['trunc']:.3e} + chain {m['chain']:.3e}; float64 {m['fd']:.6e} {m['inner']:.6e}")
    assert abs(fd - inner) <= tol
    assert abs(inner) >= 5.0 * tol                                   # (a gradient of zeros, or of the other sign, misses the tolerance)
    assert abs(m["inner"]) >= 5.0 * tol                              # ... and so it is for the reference alone


# ---- 4. probe_batch 2 against 3 ----
def test_probe_batch_two_against_three(ps):
    grid = pc.RUN_GRIDS[0]
    a, b = device_run(grid, "amplitude", 2), device_run(grid, "amplitude", 3)
    assert np.array_equal(a.loss, b.loss)
    bound = summed(pc.chain_bound_of(a.probe.astype(np.complex128), grid))
    r = pc.ratio(packed(a), packed(b), bound)
    print(f"probe_batch 2 against 3 on {grid}: worst difference / chain bound {r:.3e}")
    assert r <= 1.0


# ---- 5. bitwise ----
def test_bitwise(ps):
    from pyslice_amd import Aberrations
    grid = pc.RUN_GRIDS[0]
    D = gc.case(*grid)["D"]
    lens = Aberrations(defocus=60.0, astigmatism=25.0, astigmatism_angle=0.3)
    # a diffraction run and a Gradient() without the new flags, before anything of the new path has run in this process ...
    diff_before = npy(calculator(ps, grid, aberrations=lens, diffraction=ps.Diffraction(), probe_batch=2).run_diffraction().intensity)
    bare_calc = calculator(ps, grid, aberrations=lens, gradient=ps.Gradient(), probe_batch=2)
    bare_before = bare_calc.run_gradient(D)
    calc = calculator(ps, grid, aberrations=lens, gradient=ps.Gradient(positions=True, **FLAGS), probe_batch=2)
    first, again = calc.run_gradient(D), calc.run_gradient(D)
    for name in ("potential", "loss", "probe", "positions", "probe_position_gradient", "aberration_gradient_cartesian"):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    assert first.aberration_gradient == again.aberration_gradient and np.abs(first.aberration_gradient_cartesian).max() > 0
    same = calc.run_gradient(D, probe_positions=np.asarray(gc.PP), aberrations=Aberrations(defocus=60.0, astigmatism=25.0, astigmatism_angle=0.3))
    for name in ("potential", "loss", "probe", "positions", "probe_position_gradient", "aberration_gradient_cartesian"):
        assert getattr(first, name).tobytes() == getattr(same, name).tobytes(), name
    moved = calc.run_gradient(D, probe_positions=np.asarray(gc.PP) + 0.2, aberrations=Aberrations(defocus=90.0))
    assert not np.array_equal(moved.loss, first.loss)
    # ... and after a run with overrides: a new diffraction run, the same Gradient() calculator again, and the overriding
    # calculator's own engine -- put back to the lens of setup() -- in a forward run through the same probes
    diff_after = npy(calculator(ps, grid, aberrations=lens, diffraction=ps.Diffraction(), probe_batch=2).run_diffraction().intensity)
    assert diff_before.tobytes() == diff_after.tobytes()
    bare_calc.run_gradient(D, probe_positions=np.asarray(gc.PP) + 0.2, aberrations=Aberrations(defocus=90.0))
    bare_after = bare_calc.run_gradient(D)
    assert bare_before.probe is None and bare_before.probe_position_gradient is None and bare_before.aberration_gradient is None
    for name in ("potential", "loss"):
        assert getattr(bare_before, name).tobytes() == getattr(bare_after, name).tobytes(), name
        assert getattr(bare_before, name).tobytes() == getattr(first, name).tobytes(), name
    after = calc.run_gradient(D)                                     # the overrides are gone
    for name in ("potential", "loss", "probe_position_gradient", "aberration_gradient_cartesian"):
        assert getattr(first, name).tobytes() == getattr(after, name).tobytes(), name
    # without the new flags: today's results, and the shared ones are the same with and without
    plain = calculator(ps, grid, aberrations=lens, gradient=ps.Gradient(positions=True, probe=True), probe_batch=2).run_gradient(D)
    assert plain.probe_position_gradient is None and plain.aberration_gradient is None
    for name in ("potential", "loss", "probe", "positions"):
        assert getattr(first, name).tobytes() == getattr(plain, name).tobytes(), name


# ---- 6. descent ----
@pytest.mark.parametrize("kind", ["positions", "defocus"])
def test_descent(ps, kind):
    from pyslice_amd import Aberrations
    grid = pc.RUN_GRIDS[0]
    want, bound = pc.descent64(kind, grid)
    D, V = pc.descent_data(grid), uploaded(grid)
    calc = calculator(ps, grid, aberrations=Aberrations(defocus=pc.DEFOCUS_TRUE),
                      gradient=ps.Gradient(probe_positions=True, aberrations=True), probe_batch=2)
    xy, lens = np.asarray(gc.PP, dtype=np.float64), Aberrations(defocus=pc.DEFOCUS_TRUE)
    if kind == "positions":
        xy = xy + pc.SHIFT
    else:
        lens = Aberrations(defocus=pc.DEFOCUS_TRUE + pc.DEFOCUS_OFF)
    got = []
    for k in range(4):
        res = calc.run_gradient(D, potential=V, probe_positions=xy, aberrations=lens)
        got.append(res.total)
        if kind == "positions":
            xy = res.probe_position_step(xy, pc.RATE_XY)
        else:
            lens = res.aberration_step(lens, {"C10": pc.RATE_C10})
    got = np.array(got)
    print(f"descent {kind} {grid}: device losses {' '.join(f'{v:.6e}' for v in got)}; float64 {' '.join(f'{v:.6e}' for v in want)}; "
          f"worst |difference| / loss bound {(np.abs(got - want) / bound).max():.3e}")
    assert (np.abs(got - want) <= bound).all()
    assert (np.diff(got) < 0).all() and (np.diff(want) < 0).all()
    assert lens.C12 == 0.0 and lens.C30 == 0.0                       # (a rate by name moves that field alone)


# ---- 7. refusals at the engine level ----
def test_engine_refusals():
    case = pc.CHAIN_CASES[0]
    g0 = pc.white_g0(case)
    eng = engine(case.nx, case.ny, 3)
    with pytest.raises(RuntimeError, match="msl_set_probes"):
        eng.adjoint_probe_params(g0)                                 # no probes at all
    eng.set_probes(case.mrad, pc.PP)
    got = eng.adjoint_probe_params(g0)
    with pytest.raises(RuntimeError, match="msl_adjoint_add"):
        eng.adjoint_probe_params()                                   # no probe gradient in the work buffer
    with pytest.raises(ValueError, match="probes"):
        eng.adjoint_probe_params(B=4)                                # more than the handle has
    eng.upload_probes(np.ones((3, case.nx, case.ny), dtype=np.complex64))
    with pytest.raises(RuntimeError, match="msl_set_probes"):
        eng.adjoint_probe_params(g0)
    eng.set_probes(case.mrad, pc.PP)
    assert eng.adjoint_probe_params(g0).tobytes() == got.tobytes()
    eng.set_probe_members(case.mrad, pc.PP, [0.0, 10.0, -10.0])
    with pytest.raises(RuntimeError, match="msl_set_probes"):
        eng.adjoint_probe_params(g0)
    eng.set_probes(case.mrad, pc.PP)
    eng.set_aberrations(pc.aberr())                                  # the probes on the device are not these
    with pytest.raises(RuntimeError, match="msl_set_probes"):
        eng.adjoint_probe_params(g0)
    eng.set_aberrations(None)
    eng.set_probes(case.mrad, pc.PP)
    assert eng.adjoint_probe_params(g0).tobytes() == got.tobytes()
    assert eng.adjoint_probe_params_time(2) > 0.0
    eng.set_probes(0.0, pc.PP)                                       # plane waves
    with pytest.raises(RuntimeError, match="msl_set_probes"):
        eng.adjoint_probe_params(g0)
