"""White-spectrum parity of the slice loop backwards on the MI355X: adjoint_residual_kernel,
adjoint_step_kernel<VEC>, adjoint_conjprop_kernel, the store hook and the wave stack through msl_adjoint_add, on white probes,
potentials, data and weights (tools/white_parity.py: gradient_case), against pyslice_amd/adjoint.py in float64 under the case's tilted
propagator: the probe gradient of every add, every slice of the accumulator and the loss per probe, each per image, per line and per
pixel.  The bounds are composed in gradient_data() from the white-noise contract of the two-pass kernels (its docstring); nothing
here is taken from a measurement: tests/test_white_gradient_host.py holds a complex64 model of the loop to a third of them and shows
which faults they see.  The grids (none above 256 x 64 pixels): 24 x 20 x 1 (one partial tile in both kernels, no propagator), 45 x 63 x 3 on
fft_path=1 (odd pitch: the 8-byte step) and 101 x 97 x 3 (pitch 114: the 16-byte step, its pad pixel and 8-byte tail store) with all
three losses and the asymmetric white weight, 96 x 80 x 4, 256 x 64 x 2, 64 x 256 x 3, 12 x 1050 x 2 (525 pairs per row: tile boundaries inside
rows); the tilt (0.17, -0.11) wherever there is a propagator; P = 3 with adds of 3 and 2 on new probes, and P = 1.
The last test is the calculator's wiring of tilt= and aberrations= into run_gradient() on the physical inputs of gradient_cases.py."""
import importlib.util
import os

import numpy as np
import pytest

import gradient_cases as gc

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)

SEEN = {}                                       # grid -> (pitch, vec) of every case run, for the last assertion of the lists
MOVED_MIN = 0.5                                 # "of order 1": the float64 definition itself moves by 1.0 to 1.2 on these cases (host test)


def report(tag, res):
    sl, so = np.max(res["slices"], axis=0), np.max(res["slices_of"], axis=0)
    po, lo = np.max(res["probe_of"], axis=0), max(v.max() for v in res["loss_of"])
    print(f"{tag}: accumulator E_img E_line E_pix " + " ".join(f"{v:.2e}" for v in sl) + " of bound " + " ".join(f"{v:.3f}" for v in so) +
          " | probe gradient " + " ".join(f"{v:.2e}" for v in np.max(res["probe"], axis=0)) + " of bound " + " ".join(f"{v:.3f}" for v in po) +
          f" | loss of bound {lo:.3f}" + (f" | pitch {res['pitch']} vec {res['vec']} kappa {res['kappa']:.2f}" if "pitch" in res else "") +
          (" | moved " + " ".join(f"{v:.2f}" for v in res["moved"]) if "moved" in res else ""))


def check(c, res):
    report(wp.gradient_id(c), res)
    assert res["kappa"] <= wp.KAPPA_CAP
    assert (res["pitch"], res["vec"]) == wp.step_layout(c.nx, c.ny, c.fft_path)
    SEEN[(c.nx, c.ny, c.fft_path)] = (res["pitch"], res["vec"])
    for s, r in enumerate(res["slices_of"]):
        assert max(r) <= 1.0, (s, r)
    for a, r in enumerate(res["probe_of"]):
        assert max(r) <= 1.0, (a, r)
    for a, r in enumerate(res["loss_of"]):
        assert (r <= 1.0).all(), (a, r)
    if c.tilt is not None:
        assert min(res["moved"]) > MOVED_MIN, res["moved"]


@pytest.mark.parametrize("c", wp.GRAD_SINGLE_TILE_CASES + wp.GRAD_ODD_CASES + wp.GRAD_GRID_CASES + wp.GRAD_BATCH_CASES, ids=wp.gradient_id)
def test_white_gradient(c):
    check(c, wp.gradient_case(c))


def test_tilt_set_back_on_the_same_handle():
    c = wp.GRAD_RESTORE_CASE
    res = wp.gradient_case(c, restore=True)
    check(c, res)
    report("(0, 0) again " + wp.gradient_id(c), res["restored"])
    assert res["restored"]["worst"] <= 1.0


def test_the_lists_reached_both_step_variants():
    """after the cases above: the 8-byte and the 16-byte step both ran, as the handle reports them"""
    if not SEEN:
        for c in (wp.GRAD_ODD_CASES[0], wp.GRAD_ODD_CASES[3]):
            check(c, wp.gradient_case(c))
    assert {v[1] for v in SEEN.values()} == {True, False}, SEEN
    assert SEEN[(45, 63, 1)] == (63, False) and SEEN[(101, 97, 0)] == (114, True)


@pytest.mark.parametrize("what", ["tilt", "aberrations"])
def test_calculator_wiring(what):
    """MultisliceCalculator(gradient=..., tilt=...) and (..., aberrations=...) on the physical inputs of gradient_cases.py (96 x 80 x 4,
    three probes at probe_batch=2) against adjoint.py with the tilted propagator / the aberrated probes, under gradient_bound and
    loss_bound: the settings reach the handle, in an order that keeps them (precision is the white cases' business)"""
    import pyslice_amd as ps
    from pyslice_amd.adjoint import potential_gradient
    from pyslice_amd.tilt import Tilt, tilted_propagator
    grid = gc.CASES[3]
    c = gc.case(*grid)
    nx, ny, nz = grid
    dx, dy, dz = c["xs"][1] - c["xs"][0], c["ys"][1] - c["ys"][0], c["zs"][1] - c["zs"][0]
    lam = gc.orc.wavelength(gc.EV)
    probes, prop, kw = c["probes"], c["prop"], {}
    if what == "tilt":
        kw["tilt"] = Tilt(40.0, -25.0)
        prop = tilted_propagator(nx, ny, dx, dy, lam, dz, kw["tilt"])
    else:
        kw["aberrations"] = ps.Aberrations(defocus=150.0, Cs=2.0e5, astigmatism=60.0, astigmatism_angle=0.4)
        kx, ky = np.fft.fftfreq(nx, dx)[:, None], np.fft.fftfreq(ny, dy)[None, :]
        probes = np.fft.ifft2(np.fft.fft2(probes, axes=(-2, -1)) * np.exp(-1j * kw["aberrations"].chi(kx, ky, lam))[None], axes=(-2, -1))
    grad, L, pg, det = potential_gradient(probes, c["V"], c["D"], c["sigma"], prop, details=True)
    ref = dict(grad=grad, loss=L, probe=pg, **det)
    plain = gc.reference(*grid)
    calc = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(probe=True), probe_batch=2, **kw)
    calc.setup(gc.trajectory(*grid), aperture=30.0, voltage_eV=gc.EV, probe_positions=gc.PP, sampling=0.1, slice_thickness=1.0)
    res = calc.run_gradient(c["D"], potential=np.ascontiguousarray(np.moveaxis(c["V"], 0, 2)))
    got = np.moveaxis(res.potential, 2, 0)
    err, bound = np.abs(got - ref["grad"]).sum(axis=(-2, -1)), gc.gradient_bound(c, ref)
    lerr, lbound = np.abs(res.loss - ref["loss"]), gc.loss_bound(c, ref, "amplitude")
    perr = np.sqrt((np.abs(res.probe - ref["probe"]) ** 2).sum(axis=(-2, -1)) / (np.abs(ref["probe"]) ** 2).sum(axis=(-2, -1)))
    seen = np.abs(ref["grad"] - plain["grad"]).sum(axis=(-2, -1)) / gc.gradient_bound(c, plain)
    print(f"calculator {what} {grid}: gradient ||got - want||_1 / bound {(err / bound).max():.3e}; loss / bound {(lerr / lbound).max():.3e}; "
          f"probe gradient rel-L2 {perr} (3e-4); the setting moves the gradient by {seen.max():.3g} bounds")
    assert seen.max() > 100.0                                       # (the setting is seen by this bound)
    assert (err <= bound).all(), err / bound
    assert (lerr <= lbound).all(), lerr / lbound
    assert (perr <= 3.0 * gc.EPS).all()
