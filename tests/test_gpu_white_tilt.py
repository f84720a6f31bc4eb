"""White-spectrum parity of the slice-loop pass kernels on TILTED propagator tables, per image, per line and per pixel
(tools/white_parity.py with tilt=).

Without a tilt every Fresnel table of the slice loop is even in k, P[m] = P[n - m]: a pass that reads its table at -k, mirrors half
of it or gets the sign of the Nyquist bin wrong computes the same numbers, and no test on untilted tables can tell.  A tilt puts a
linear phase on the table (csrc/propagator.h, msl_set_tilt) and ends that.  tests/test_gpu_tilt.py checks the tilted tables on eight
grids with 30 mrad probes and one energy-weighted norm, which is blind to the outer nine tenths of k-space; here the input is white
(test_gpu_white_spectrum.py), the tangents are (0.17, -0.11) -- 0.85 px and -0.55 px per slice, fractional on both axes -- and the
reference is the float64 definition of pyslice_amd/tilt.py.  In float64, on these inputs, a table mirrored on one axis or left
untilted gives E_img 1.3 - 1.5, a wrong Nyquist sign 3e-2 - 5e-2, one entry off by 1e-3 rad 3e-5 - 9e-5
(tests/test_white_tilt_host.py); the E_img bounds here are 3e-6 - 2.7e-5.

Bounds: those of test_gpu_white_spectrum.py, unchanged (wp.bounds: tol sqrt(n_t) x (1, 2, 10), tol = 3e-6 with both axes on a direct
kernel, 1e-5 otherwise).  A tilt only changes the values in tables that are rounded to float once, so a tilted pass is owed no more
error than an untilted one.  The spectrum tapped after slice k has seen 2 k transforms of the loop and its own: n_t = 2 k + 1.
Where the tilt lies along an axis whose one-pass kernel needs an even table the loop runs on the two-pass kernels, the kernel set of
test_fft2_matches_numpy, with its contract: 3e-6 when both lengths are 13-smooth, else 1e-5.

Every tilted result must also be more than 1 (rel-L2) away from the UNTILTED float64 reference: two white fields shifted against
each other by a fraction of a pixel per slice are nearly uncorrelated (1.35 - 1.41 with both axes tilted, 1.16 - 1.29 with one).
`python tools/white_parity.py --tilt-only profiles/white_tilt_parity.txt` records the measured figures per kernel family (a record:
no bound is taken from it).
"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)


def _ids(cases):
    name = {wp.TILT: "xy", wp.TILT_X: "x", wp.TILT_Y: "y"}
    return ["x".join(str(v) for v in c[:3]) + "-tilt_" + name[c[3]] for c in cases]


def _within(tag, m, lim):
    print(f"{tag}: E_img {m[0]:.3e} E_line {m[1]:.3e} E_pix {m[2]:.3e} (bounds {lim[0]:.2e} {lim[1]:.2e} {lim[2]:.2e})")
    return [f"{tag} {what} {v:.3e} above {b:.3e}" for what, v, b in zip(("E_img", "E_line", "E_pix"), m, lim) if not v <= b]


def _check(nx, ny, nz, tilt):
    """a case that stays on the one-pass loop under its tilt"""
    res = wp.white_case(nx, ny, nz, tilt=tilt)
    print(f"{nx} x {ny} x {nz} tilt {tilt}: one-pass {res['one_pass']}, {res['moved']:.3f} from the untilted reference")
    above = [msg for name in ("exit", "spectrum") for msg in _within(name, res[name], wp.bounds(nx, ny, nz, name == "spectrum"))]
    assert res["one_pass"], "the slice loop did not run its one-pass kernels on this grid under the tilt"
    assert res["moved"] > 1.0, "the tilt did not move the wave"
    assert not above, above


def test_the_tilt_lists_cover_every_kernel():
    from pyslice_amd import _native
    assert len(wp.MIXED_LENGTHS) == 99
    assert {c[0] for c in wp.TILT_MIXED_CASES if c[1] == 135 and c[2] == 3} == set(wp.MIXED_LENGTHS)
    assert {c[1] for c in wp.TILT_MIXED_CASES if c[0] == 135 and c[2] == 2} == set(wp.MIXED_LENGTHS)
    assert all(c[3] == wp.TILT for c in wp.TILT_MIXED_CASES + wp.TILT_POW2_CASES + wp.TILT_GENERIC_CASES)
    assert all(_native.line_kernel_class(n) == 1 for n in wp.MIXED_LENGTHS + [135, 144])
    # the generic lengths: no direct kernel, and not a convolution length either (below 33, or 13-smooth in 129..191)
    assert wp.GENERIC_LENGTHS == [16, 32, 143, 169, 176, 182]
    assert all(_native.line_kernel_class(n) == 0 and wp.family(n, 135) == wp.family(n, 144) == "generic one-pass" for n in wp.GENERIC_LENGTHS)
    for cross in (135, 144):
        assert {c[0] for c in wp.TILT_GENERIC_CASES if c[1] == cross} == {c[1] for c in wp.TILT_GENERIC_CASES if c[0] == cross} == set(wp.GENERIC_LENGTHS)
    # four-step R = 16 and 32 and the 2 R^2 kernel, each on both axes and paired with a register kernel
    for n in (256, 1024, 512):
        assert (n, 144, 3, wp.TILT) in wp.TILT_POW2_CASES and (144, n, 2, wp.TILT) in wp.TILT_POW2_CASES
    assert all(wp.family(*wp.axis_under_test(*c[:2])) in ("four-step", "2R^2") for c in wp.TILT_POW2_CASES)
    # every convolution length M (256, 1024, 2048, and the even-odd layout of 4096) on a device-written filter, and the wave kernel
    fams = {wp.family(n, 144) for n in wp.TILT_CROSS_LENGTHS}
    assert fams == {"convolution 256", "convolution 1024", "convolution 2048", "convolution 4096", "wave-2K"}
    assert set(wp.TILT_CROSS_LENGTHS) == {n for n in wp.CONV_LENGTHS if wp.family(n, 144).startswith("convolution")} | {2048}
    for n in wp.TILT_CROSS_LENGTHS:
        assert (n, 144, 3, wp.TILT_Y) in wp.TILT_CROSS_CASES and (144, n, 2, wp.TILT_X) in wp.TILT_CROSS_CASES
    # the fallback cases tilt the axis that needs an even table, and both contracts give them the same tolerance
    for nx, ny, nz, tilt in wp.TILT_FALLBACK_CASES:
        n, other = (nx, ny) if tilt == wp.TILT_X else (ny, nx)
        assert other == 144 and (wp.family(n, other).startswith("convolution") or wp.family(n, other) == "wave-2K")
        assert wp.two_pass_tolerance(nx, ny) == wp.tolerance(nx, ny)
    assert wp.bounds(600, 135, 4, True, layer=3) == wp.bounds(600, 135, 4, True)          # the exit is the tap after the last slice
    assert wp.bounds(600, 135, 4, True, layer=0) == wp.bounds(600, 135, 1, False)         # one transform: one tolerance


@pytest.mark.parametrize("nx,ny,nz,tilt", wp.TILT_MIXED_CASES, ids=_ids(wp.TILT_MIXED_CASES))
def test_every_mixed_radix_length_on_tilted_tables(nx, ny, nz, tilt):
    """each of the 99 rowTM / rowTM2 instantiations along x (nz = 3) and along y (nz = 2) against 135 lines, both axes tilted"""
    _check(nx, ny, nz, tilt)


@pytest.mark.parametrize("nx,ny,nz,tilt", wp.TILT_POW2_CASES, ids=_ids(wp.TILT_POW2_CASES))
def test_register_kernels_on_tilted_tables(nx, ny, nz, tilt):
    """four-step R = 16 / 32 and the 2 R^2 kernel with its split-order table, on both axes, against a mixed-radix cross axis and
    paired with each other (alternating scheme, interleaved work-buffer order)"""
    _check(nx, ny, nz, tilt)


@pytest.mark.parametrize("nx,ny,nz,tilt", wp.TILT_GENERIC_CASES, ids=_ids(wp.TILT_GENERIC_CASES))
def test_generic_one_pass_kernel_on_tilted_tables(nx, ny, nz, tilt):
    """AX_GENERIC is not among the even-table kinds of tilt_needs_two_pass: it runs one-pass under any tilt"""
    _check(nx, ny, nz, tilt)


@pytest.mark.parametrize("nx,ny,nz,tilt", wp.TILT_CROSS_CASES, ids=_ids(wp.TILT_CROSS_CASES))
def test_even_axis_on_device_written_tables_and_filters(nx, ny, nz, tilt):
    """the tilt along the 144-point axis only: the convolution axis (every M, rowTB / rowTB2 / rowTC2) and the 2048-point wave
    kernel read the even table, and the filter, that conv_lag_kernel / conv_filter_kernel wrote after msl_set_tilt"""
    _check(nx, ny, nz, tilt)


@pytest.mark.parametrize("nx,ny,nz,tilt", wp.TILT_FALLBACK_CASES, ids=_ids(wp.TILT_FALLBACK_CASES))
def test_tilt_along_an_even_table_axis_takes_the_two_pass_loop_and_comes_back(nx, ny, nz, tilt):
    res = wp.white_case(nx, ny, nz, tilt=tilt, restore=True)
    back = res["restored"]
    print(f"{nx} x {ny} x {nz} tilt {tilt}: one-pass {res['one_pass']}, {res['moved']:.3f} from the untilted reference; "
          f"after (0, 0): one-pass {back['one_pass']}")
    above = []
    for name in ("exit", "spectrum"):
        above += _within(name, res[name], wp.bounds(nx, ny, nz, name == "spectrum", tol=wp.two_pass_tolerance(nx, ny)))
        above += _within("(0, 0) again " + name, back[name], wp.bounds(nx, ny, nz, name == "spectrum"))
    assert not res["one_pass"], "a tilt along an axis that needs an even table ran on the one-pass loop"
    assert back["one_pass"], "set_tilt(0, 0) did not bring the one-pass loop back"
    assert res["moved"] > 1.0, "the tilt did not move the wave"
    assert not above, above


@pytest.mark.parametrize("nx,ny,nz,tilt,layers", wp.TILT_LAYER_CASES, ids=_ids(wp.TILT_LAYER_CASES))
def test_layer_taps_on_tilted_tables(nx, ny, nz, tilt, layers):
    """the taps after slices 0, 1, 2 of 4 read the output of passes along y and along x (conj P_y in the row FFT, conj P_x in the
    epilogue), in natural and interleaved line order; 501 x 144 with the tilt along x is the tap of the two-pass loop"""
    res = wp.white_case(nx, ny, nz, tilt=tilt, layers=layers)
    print(f"{nx} x {ny} x {nz} tilt {tilt}: one-pass {res['one_pass']}, exit {res['moved']:.3f} from the untilted reference, taps " +
          ", ".join(f"{k} ({wp.tap_axis(nx, ny, nz, k, res['one_pass'])}): {res['layers_moved'][k]:.3e}" for k in layers))
    above = [msg for name in ("exit", "spectrum") for msg in _within(name, res[name], wp.bounds(nx, ny, nz, name == "spectrum"))]
    for k in layers:
        above += _within(f"tap after slice {k}", res["layers"][k], wp.bounds(nx, ny, nz, True, layer=k))
    above += _within("exit of the tapped run", res["layers_exit"], wp.bounds(nx, ny, nz, True))
    # nothing is propagated before slice 0: its spectrum is that of the untilted run; every later one has moved
    above += _within("tap after slice 0 against the untilted reference", res["layers_untilted"][0], wp.bounds(nx, ny, nz, True, layer=0))
    assert res["one_pass"] == (tilt == wp.TILT)
    assert res["moved"] > 1.0 and all(res["layers_moved"][k] > 1.0 for k in layers if k > 0)
    assert {wp.tap_axis(nx, ny, nz, k, res["one_pass"]) for k in layers} == ({"x", "y"} if res["one_pass"] else {"two-pass"})
    assert not above, above
