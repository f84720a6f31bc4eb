"""Gradients on the host: the float64 definition (pyslice_amd/adjoint.py) against its own tangent and finite differences, the fault
sensitivity of the bounds test_gpu_gradient.py puts on the device (on its exact inputs, tests/gradient_cases.py), the calculator's
call order on the recording engine, and the ABI."""
import os
import re

import numpy as np
import pytest

import gradient_cases as gc
from recording_engine import RecordingEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AX = (-2, -1)


def small(seed=0, nx=24, ny=20, nz=3, P=2):
    from pyslice_amd.tilt import tilted_propagator
    rng = np.random.default_rng(seed)
    probes = rng.standard_normal((P, nx, ny)) + 1j * rng.standard_normal((P, nx, ny))
    probes /= np.sqrt((np.abs(probes) ** 2).sum(axis=AX))[:, None, None]
    V = rng.standard_normal((nz, nx, ny))
    sigma = 0.3
    prop = tilted_propagator(nx, ny, 0.1, 0.1, 0.037, 1.0, None)
    return probes, V, sigma, prop, rng


def tangent(probes, V, dV, sigma, prop):
    """J dV: the analytic tangent of the exit spectra of forward_waves along dV"""
    from pyslice_amd.adjoint import forward_waves
    psis, phis, _ = forward_waves(probes, V, sigma, prop)
    dpsi = np.zeros_like(psis[0])
    for s in range(V.shape[0]):
        t = np.exp(1j * sigma * V[s])[None]
        dphi = t * dpsi + 1j * sigma * dV[s][None] * phis[s]
        if s < V.shape[0] - 1:
            dpsi = np.fft.ifft2(prop[None] * np.fft.fft2(dphi, axes=AX), axes=AX)
    return np.fft.fft2(dphi, axes=AX)


def test_adjoint_identity():
    """<J dV, r> = <dV, J^H r> in the real inner product 2 Re sum conj(r) J dV (the convention dL = 2 Re sum conj(G) dPsi): the
    backward loop fed the residual r is J^H r; the tangent is checked against central differences of forward_waves first"""
    from pyslice_amd.adjoint import backward, forward_waves
    probes, V, sigma, prop, rng = small()
    dV = rng.standard_normal(V.shape)
    r = rng.standard_normal(probes.shape) + 1j * rng.standard_normal(probes.shape)
    J = tangent(probes, V, dV, sigma, prop)
    h = 1e-5
    fd = (forward_waves(probes, V + h * dV, sigma, prop)[2] - forward_waves(probes, V - h * dV, sigma, prop)[2]) / (2 * h)
    assert np.linalg.norm(fd - J) <= 1e-8 * np.linalg.norm(J)
    psis = forward_waves(probes, V, sigma, prop)[0]
    JHr = backward(r, psis, V, sigma, prop)[0]
    lhs, rhs = 2.0 * (np.conj(r) * J).real.sum(), (dV * JHr).sum()
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize("loss", gc.LOSSES)
def test_finite_differences(loss):
    from pyslice_amd.adjoint import forward_waves, potential_gradient, total_loss
    probes, V, sigma, prop, rng = small(1)
    data = np.fft.fftshift(np.abs(forward_waves(probes, 0.9 * V, sigma, prop)[2]) ** 2, axes=AX)
    eps = 1e-20 if loss != "poisson" else 1e-6
    grad, L, pg = potential_gradient(probes, V, data, sigma, prop, loss=loss, epsilon=eps)
    assert L.shape == (2,) and grad.shape == V.shape and pg.shape == probes.shape
    for s, x, y in zip(rng.integers(0, 3, 8), rng.integers(0, 24, 8), rng.integers(0, 20, 8)):
        # Richardson: the h^2 term of the central difference taken out
        def cd(h):
            e = np.zeros_like(V); e[s, x, y] = h
            return (total_loss(probes, V + e, data, sigma, prop, loss, None, eps) - total_loss(probes, V - e, data, sigma, prop, loss, None, eps)) / (2 * h)
        fd = (4.0 * cd(5e-4) - cd(1e-3)) / 3.0
        assert abs(fd - grad[s, x, y]) <= 1e-6 * abs(grad[s, x, y]), (loss, s, x, y, fd, grad[s, x, y])


def test_probe_gradient_and_weight():
    """the probe gradient is dL/dpsi_0*: dL = 2 Re sum conj(pg) dpsi_0; a weight of zero takes a pixel out of loss and gradient"""
    from pyslice_amd.adjoint import forward_waves, potential_gradient, total_loss
    probes, V, sigma, prop, rng = small(2)
    data = np.fft.fftshift(np.abs(forward_waves(probes, 0.9 * V, sigma, prop)[2]) ** 2, axes=AX)
    w = (rng.random(V.shape[1:]) > 0.3).astype(np.float64)
    grad, L, pg = potential_gradient(probes, V, data, sigma, prop, weight=w)
    d = rng.standard_normal(probes.shape) + 1j * rng.standard_normal(probes.shape)
    h = 1e-6
    fd = (total_loss(probes + h * d, V, data, sigma, prop, weight=w) - total_loss(probes - h * d, V, data, sigma, prop, weight=w)) / (2 * h)
    assert abs(fd - 2.0 * (np.conj(pg) * d).real.sum()) <= 1e-6 * abs(fd)
    data2 = data.copy()
    data2[:, w == 0] += 1.0
    grad2, L2, _ = potential_gradient(probes, V, data2, sigma, prop, weight=w)
    assert np.array_equal(grad, grad2) and np.array_equal(L, L2)


# ---- the faults the device bounds must see ----
FAULTS = ("conj_P", "conj_t", "phi_psi", "scale_N", "shift")


def faulty_gradient(c, ref, fault):
    """the backward loop of the definition with one fault built in -> grad (nz, nx, ny)"""
    V, sigma, prop, psis = c["V"], c["sigma"], c["prop"], ref["psi"]
    nz, nx, ny = V.shape
    G = ref["G"]
    if fault == "shift":                    # the detector layout mapped with (n - 1) / 2 + 1 where n / 2 belongs: off by one on odd nx
        from pyslice_amd.adjoint import loss_and_residual
        G = loss_and_residual(ref["Psi"], np.roll(c["D"], 1 if nx % 2 else 0, axis=1), "amplitude")[1]
    g = (1.0 if fault == "scale_N" else nx * ny) * np.fft.ifft2(G, axes=AX)
    grad = np.zeros_like(V)
    for s in range(nz - 1, -1, -1):
        t = np.exp(1j * sigma * V[s])[None]
        phi = psis[s] if fault == "phi_psi" else t * psis[s]
        grad[s] = 2.0 * sigma * (g * np.conj(phi)).imag.sum(axis=0)
        if fault != "conj_t":
            g = np.conj(t) * g
        if s > 0:
            g = np.fft.ifft2((prop if fault == "conj_P" else np.conj(prop))[None] * np.fft.fft2(g, axes=AX), axes=AX)
    return grad


@pytest.mark.parametrize("grid", gc.CASES)
def test_device_bounds_see_every_fault(grid):
    """on the inputs of test_gpu_gradient.py every fault of the backward loop, where the grid can show it (a propagator and a second
    slice for conj(P) and conj(t), an odd nx for the shift), misses the per-slice bound of the device test by a factor of 10 or more
    in some slice (the device test asserts every slice).  The faults are built into the amplitude loss without a weight: the other
    two losses and the weighted runs share the backward loop and are not fault-checked here."""
    nx, ny, nz = grid
    c, ref = gc.case(*grid), gc.reference(*grid)
    bound = gc.gradient_bound(c, ref)
    assert np.abs(faulty_gradient(c, ref, None) - ref["grad"]).max() == 0.0
    for fault in FAULTS:
        if (fault in ("conj_P", "conj_t") and nz < 2) or (fault == "shift" and nx % 2 == 0):
            continue
        err = np.abs(faulty_gradient(c, ref, fault) - ref["grad"]).sum(axis=AX)
        print(f"fault {fault} {grid}: worst ||fault - want||_1 / bound over the slices {(err / bound).max():.3e}")
        assert (err / bound).max() >= 10.0, (fault, grid, err / bound)


def test_direction_step_of_the_device_test():
    """the float64 side of test_directional_derivative: at the h the device test uses, the truncation of the definition's central
    difference is below a hundredth of the device test's loss term, the two loss bounds over 2h"""
    from pyslice_amd.adjoint import directional_check
    grid = gc.CASES[3]
    c, ref = gc.case(*grid), gc.reference(*grid)
    d = gc.smooth_direction(*grid)
    fd, inner = directional_check(c["probes"], c["V"], c["D"], c["sigma"], c["prop"], d, gc.DIRECTION_H)
    loss_term = 2.0 * gc.loss_bound(c, ref, "amplitude").sum() / (2.0 * gc.DIRECTION_H)
    print(f"directional float64 {grid}: fd {fd:.9e} <grad, d> {inner:.9e} truncation {abs(fd - inner):.2e} loss term {loss_term:.2e}")
    assert abs(fd - inner) <= 0.01 * loss_term
    assert loss_term < abs(inner)                                   # (the check can tell the derivative from zero)


# ---- calculator logic ----
class GradientRecorder(RecordingEngine):
    def __init__(self, nx, ny, nz, *a, **k):
        super().__init__(nx, ny, nz, *a, **k)
        self._shape = (nx, ny, nz)

    def adjoint_add(self, data, B=None, probe=False):
        self.calls.append(("adjoint_add", (data,), dict(B=B, probe=probe)))
        nx, ny, _ = self._shape
        return np.arange(B, dtype=np.float64) + 1.0, (np.ones((B, nx, ny), dtype=np.complex64) if probe else None)

    def adjoint_download(self):
        self.calls.append(("adjoint_download", (), {}))
        nx, ny, nz = self._shape
        return np.arange(nz, dtype=np.float64)[:, None, None] * np.ones((nz, nx, ny))


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    made = []

    def make(*a, **k):
        made.append(GradientRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(_native, "Engine", make)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    return made


def setup_calc(ps, recorder, n_probes=5, **kw):
    tr = gc.trajectory(96, 80, 4)
    pp = [(1.0 + 0.5 * i, 2.0) for i in range(n_probes)]
    calc = ps.MultisliceCalculator(device=0, progress=False, **kw)
    calc.setup(tr, aperture=30.0, voltage_eV=gc.EV, probe_positions=pp, sampling=0.1, slice_thickness=1.0)
    return calc, recorder[-1]


def test_calculator_call_order_and_ragged_batch(recorder):
    import pyslice_amd as ps
    calc, eng = setup_calc(ps, recorder, gradient=ps.Gradient(loss="intensity", probe=True), probe_batch=2)
    assert eng.n_probes == 2 and eng.frame_batch == 1
    names = [c[0] for c in eng.calls]
    assert "set_adjoint" in names and names.index("set_adjoint") > names.index("set_slices")
    a = [c for c in eng.calls if c[0] == "set_adjoint"][0][1]
    assert a[0] == 2 and a[1] == 1e-20 and a[2] is None
    eng.calls.clear()
    data = np.ones((5, 96, 80))
    res = calc.run_gradient(data)
    names = [c[0] for c in eng.calls]
    assert names == ["build_potential", "adjoint_reset"] + ["set_probes", "adjoint_add"] * 3 + ["adjoint_download"]
    adds = [c for c in eng.calls if c[0] == "adjoint_add"]
    assert [c[2]["B"] for c in adds] == [2, 2, 1] and [c[1][0].shape[0] for c in adds] == [2, 2, 1]      # the ragged last batch
    assert all(c[2]["probe"] for c in adds)
    sets = [c for c in eng.calls if c[0] == "set_probes"]
    assert all(c[1][1].shape == (2, 2) for c in sets)             # padded to the engine's probe count
    assert res.potential.shape == (96, 80, 4) and res.potential[3, 5, 2] == 2.0
    assert res.loss.tolist() == [1.0, 2.0, 1.0, 2.0, 1.0] and res.total == 7.0
    assert res.probe.shape == (5, 96, 80) and res.kind == "intensity"
    V = np.zeros((96, 80, 4))
    assert np.array_equal(res.descent_step(V, 0.5), -0.5 * res.potential)
    with pytest.raises(ValueError):
        res.descent_step(np.zeros((4, 96, 80)), 0.5)


def test_calculator_potential_upload_and_data_checks(recorder):
    import pyslice_amd as ps
    calc, eng = setup_calc(ps, recorder, n_probes=3, gradient=ps.Gradient())
    eng.calls.clear()
    V = np.arange(96 * 80 * 4, dtype=np.float64).reshape(96, 80, 4)
    res = calc.run_gradient(np.ones((3, 96, 80)), potential=V)
    names = [c[0] for c in eng.calls]
    assert names[0] == "upload_potential" and "build_potential" not in names
    up = eng.calls[0][1][0]
    assert up.shape == (4, 96, 80) and up.dtype == np.float32 and up[2, 5, 7] == np.float32(V[5, 7, 2])
    assert res.probe is None
    for bad in (np.ones((2, 96, 80)), np.ones((3, 80, 96))):
        with pytest.raises(ValueError, match="gradient: data"):
            calc.run_gradient(bad)
    with pytest.raises(ValueError, match="gradient: potential"):
        calc.run_gradient(np.ones((3, 96, 80)), potential=np.zeros((4, 96, 80)))
    with pytest.raises(ValueError, match="gradient: frame"):
        calc.run_gradient(np.ones((3, 96, 80)), frame=1)
    plain = ps.MultisliceCalculator(device=0, progress=False)
    with pytest.raises(RuntimeError, match="gradient="):
        plain.run_gradient(np.ones((3, 96, 80)))


def test_refusals_by_name():
    import pyslice_amd as ps
    g = ps.Gradient()
    from types import SimpleNamespace
    x = object()                            # (the refusal comes before any look at the object)
    combos = {
        "bandlimit": dict(bandlimit=x), "projection": dict(projection=x), "prism": dict(prism=x), "coherence": dict(coherence=x),
        "precession": dict(precession=x), "k_window": dict(k_window=(8, 8)), "k_bin": dict(k_bin=(2, 2)), "layers": dict(layers=[0]),
        "thickness": dict(thickness=x), "tds": dict(tds=True), "ionization": dict(ionization=x), "spectroscopy": dict(spectroscopy=x),
        "imaging": dict(imaging=x), "detectors": dict(detectors=x), "diffraction": dict(diffraction=ps.Diffraction()),
        "polar": dict(polar=x), "dose": dict(diffraction=SimpleNamespace(dose=x)), "cache": dict(cache=True),
        "stream_tile": dict(stream_tile=4), "frame_batch > 1": dict(frame_batch=2),
    }
    for what, kw in combos.items():
        with pytest.raises(NotImplementedError, match=re.escape(f"gradient: {what} is not built")):
            ps.MultisliceCalculator(device=0, progress=False, gradient=g, **kw)


def test_refusals_in_setup(monkeypatch, recorder):
    import pyslice_amd as ps
    from pyslice_amd import distributed
    tr = gc.trajectory(96, 80, 4)
    box = tr.box_matrix
    sources = {
        "FrozenPhonons": ps.FrozenPhonons(tr.atom_types, tr.positions[0], box, sigma=0.05, n_configs=2),
        "AbsorptivePotential": ps.AbsorptivePotential(tr.atom_types, tr.positions[0], box, {14: 0.078, 8: 0.09}),
        "PhononModes": ps.PhononModes(tr.atom_types, tr.positions[0], box, np.zeros(tr.n_atoms, dtype=np.int64), [[0.1, 0.0, 0.0]], [1.0],
                                      np.full((1, 1, 3), 0.01 + 0j), n_frames=2),
    }
    for what, src in sources.items():
        calc = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient())
        with pytest.raises(NotImplementedError, match=f"gradient: {what} is not built"):
            calc.setup(src, aperture=30.0, voltage_eV=gc.EV, sampling=0.1, slice_thickness=1.0)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    calc = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient())
    with pytest.raises(NotImplementedError, match="gradient: a run over several ranks is not built"):
        calc.setup(tr, aperture=30.0, voltage_eV=gc.EV, sampling=0.1, slice_thickness=1.0)


def test_gradient_validation(recorder):
    import pyslice_amd as ps
    with pytest.raises(ValueError, match="loss must be one of"):
        ps.Gradient(loss="l2")
    for eps in (0.0, -1.0, np.inf, np.nan, 1e-50, 1e39):          # (the last two: zero and infinity in the float32 of the kernels)
        with pytest.raises(ValueError, match="epsilon"):
            ps.Gradient(epsilon=eps)
    for w in (np.ones(4), -np.ones((4, 4)), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError, match="weight"):
            ps.Gradient(weight=w)
    with pytest.raises(ValueError, match="expected a Gradient"):
        ps.MultisliceCalculator(device=0, progress=False, gradient="amplitude")
    g = ps.Gradient(loss="poisson", weight=np.ones((4, 4)), epsilon=1e-3, probe=True)
    assert g.kind == 3 and g.weight.dtype == np.float32 and not g.weight.flags.writeable
    with pytest.raises(ValueError, match="gradient: weight"):
        setup_calc(ps, recorder, gradient=g)


# ---- ABI ----
def test_abi():
    from pyslice_amd import _native
    header = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"#define MSL_ABI_VERSION 3\b", header) and _native.ABI_VERSION == 3
    for name in ("msl_set_adjoint", "msl_adjoint_reset", "msl_adjoint_add", "msl_adjoint_download", "msl_adjoint_step_time"):
        assert re.search(r"^int\s+" + name + r"\(msl_handle\* h", header, re.M), name
        assert name in _native.EXPORTS
    for name in ("set_adjoint", "adjoint_reset", "adjoint_add", "adjoint_download", "adjoint_step_time"):
        assert callable(getattr(_native.Engine, name))
    from pyslice_amd.adjoint import LOSSES
    for key, val in LOSSES.items():
        assert re.search(rf"MSL_ADJ_{key.upper()} = {val}\b", header)
