"""White-spectrum parity of the layer taps and of the windowed, binned, frame-scattered output (tools/white_parity.py: output_case).

The white suites of the slice-loop passes stop at the exit wave and the full-size exit spectrum.  Between a pass's work buffer and a
stored spectrum lie the tap's gather out of three line orders (natural, interleaved with rp = 16 / 32, the 2048-point paired lines),
transposed or not, the multiplication by conj(P_d) in one of four places (fast / generic row FFT, COL_MULPX of the fast column
kernel, MUL_VEC of the generic column pass), the choice of the column kernel (fast_ok), the k-window that moves whole tiles, the
out_group frame scatter and bin_stage -> bin_frames.  Physical input weights the outer nine tenths of k-space with 1e-5 of the
energy, so one rel-L2 < 1e-4 passes a window origin one tile off out there; here the probes and the potentials are white, the tables
are the untilted ones fill_propagator writes on the host, and every tap and every stored spectrum of every batch slot is compared
with the float64 reference (cropped at n/2 - w/2, block-summed coherently) per image, per line and per pixel.

Bounds: wp.bounds(nx, ny, nz, True, layer=k) for the tap after slice k, wp.bounds(nx, ny, nz, True) for the exit, with
two_pass_tolerance on the two-pass loops: the white-noise contract of test_gpu_white_spectrum.py, unchanged.  A window is a crop of
a homogeneous error field and a coherent block sum adds error and signal alike in quadrature, so the same bounds hold for the stored
form (tests/test_white_output_host.py shows it on a complex64 CPU evaluation, and that each fault of these paths exceeds them).
Every case asserts the loop it ran on (the byte count of the fused, tapped loop) and, through tap_layout(), that its list reaches
the path it is named for.  `python tools/white_parity.py --output-only profiles/white_output_parity.txt` records the figures (a
record: no bound is taken from it).
"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)


def _ids(cases):
    return [wp.output_id(c) for c in cases]


def _within(tag, m, lim):
    print(f"{tag}: E_img {m[0]:.3e} E_line {m[1]:.3e} E_pix {m[2]:.3e} (bounds {lim[0]:.2e} {lim[1]:.2e} {lim[2]:.2e})")
    return [f"{tag} {what} {v:.3e} above {b:.3e}" for what, v, b in zip(("E_img", "E_line", "E_pix"), m, lim) if not v <= b]


def _layouts(c, one_pass=None):
    one_pass = (not c.fft_path) if one_pass is None else one_pass
    return [wp.tap_layout(c.nx, c.ny, c.nz, k, one_pass, c.window, c.fft_path) for k in c.layers]


def _check(c, **kw):
    """every tap and the exit of every batch slot of a case inside its bounds, on the loop the case is listed for"""
    res = wp.output_case(*c, **kw)
    print(f"{wp.output_id(c)}: one-pass {res['one_pass']} ({res['bytes']} bytes), taps " +
          ", ".join("%d: %s %s%s, row %s, column %s" % ((k,) + lay[:2] + (f" rp {lay[2]}" if lay[2] else "",) + lay[3:]) for k, lay in zip(c.layers, _layouts(c))))
    above = []
    for b in range(c.frame_batch):
        for k in c.layers:
            above += _within(f"slot {b} tap after slice {k}", res["taps"][(b, k)], wp.case_bounds(c, k))
        above += _within(f"slot {b} exit", res["exit"][b], wp.case_bounds(c))
    assert len(res["taps"]) == c.frame_batch * len(c.layers) and len(res["exit"]) == c.frame_batch
    assert res["one_pass"] is (not c.fft_path), "the fused, tapped slice loop did not move the bytes of the loop this case is listed for"
    assert res["exit_is_last_block"], "wavefunction() is not the last block of layers_c64()"
    if c.frame_batch > 1:
        print("slot 0 against the reference of slot 1: " + ", ".join(f"{k}: {v:.3f}" for k, v in res["cross"].items()))
        assert set(res["cross"]) == set(c.layers) | {"exit"} and all(v > 1.0 for v in res["cross"].values()), res["cross"]
    assert not above, above
    return res


def test_the_plans_of_the_library_are_the_restated_ones():
    """what the library can tell of its plan agrees with axis_plan(): the direct-kernel class of every length in the lists"""
    from pyslice_amd import _native
    for _, cases in wp.OUTPUT_LISTS:
        for c in cases:
            for n, other, r in ((c.nx, c.ny, wp.plan_radices(c.nx, c.ny)[0]), (c.ny, c.nx, wp.plan_radices(c.nx, c.ny)[1])):
                p = wp.axis_plan(n, other, r)
                assert (_native.line_kernel_class(n) == 1) == (n in wp._mixed_groups()), n
                assert (p.kind == "mixed") == (_native.line_kernel_class(n) == 1), (n, other)
                assert p.kind not in ("fourstep", "two", "wave2k") or _native.line_kernel_class(n) == 2, (n, other)


@pytest.mark.parametrize("c", wp.OUT_UNTILTED_CASES, ids=_ids(wp.OUT_UNTILTED_CASES))
def test_taps_on_the_host_filled_conjugate_tables(c):
    """the grids of TILT_LAYER_CASES without a tilt: tap_cx / tap_cy as fill_propagator derives them and copy_table writes them.
    501 x 144 is one-pass here: the tap behind a convolution axis"""
    _check(c)
    assert {lay[0] for lay in _layouts(c)} == {"x", "y"}


@pytest.mark.parametrize("c", wp.OUT_ALTERNATING_CASES, ids=_ids(wp.OUT_ALTERNATING_CASES))
def test_taps_of_the_alternating_scheme_at_both_parities_and_radices(c):
    """256 / 1024 on both axes: interleaved order up to k = nz - 3 and natural order at nz - 2 at both parities of nz, rp 16 and
    32 in one run with COL_MULPX on both radices; 256 x 144 (ny % 32 = 16) sends conj(P_x) through MUL_VEC of the generic pass"""
    _check(c)
    lay = _layouts(c)
    if c.ny == 144:
        assert ("x", "natural", 0, "generic", "generic") in lay and wp.plan_radices(c.nx, c.ny) == (16, 0)
    else:
        assert [l[1] for l in lay] == ["interleaved"] * (c.nz - 2) + ["natural"] and all(l[3:] == ("fast", "fast") for l in lay)
        assert {l[2] for l in lay if l[2]} == ({16, 32} if c.nx != c.ny else {16})


@pytest.mark.parametrize("c", wp.OUT_SCHEME_B_CASES, ids=_ids(wp.OUT_SCHEME_B_CASES))
def test_taps_in_interleaved_order_between_unequal_radices(c):
    """512 against 256 / 1024: every pass transposes, every tap gathers the interleaved order of the READING kernel"""
    _check(c)
    lay = _layouts(c)
    assert all(l[1] == "interleaved" for l in lay)
    assert [l[2] for l in lay] == [32 if (c.nx if l[0] == "y" else c.ny) == 1024 else 16 for l in lay]


@pytest.mark.parametrize("c", wp.OUT_PAIRED_CASES, ids=_ids(wp.OUT_PAIRED_CASES))
def test_taps_out_of_the_paired_lines_order(c):
    """2048 x 2048: both axes on the wave kernel, the work buffer between two passes holds its lines in pairs"""
    _check(c)
    assert [l[:2] for l in _layouts(c)] == [("y", "paired"), ("x", "paired"), ("y", "paired")]


@pytest.mark.parametrize("c", wp.OUT_WAVE_NATURAL_CASES + wp.OUT_ROWTM2_CASES + wp.OUT_MIXED16_CASES,
                         ids=_ids(wp.OUT_WAVE_NATURAL_CASES + wp.OUT_ROWTM2_CASES + wp.OUT_MIXED16_CASES))
def test_taps_behind_the_wave_kernel_and_the_mixed_radix_kernels(c):
    """natural order out of the 2048-point wave kernel, of rowTM2 (G = 64, 1000 points) and of a G = 16 mixed-radix kernel"""
    _check(c)
    assert [l[:2] for l in _layouts(c)] == [("y", "natural"), ("x", "natural"), ("y", "natural")]


@pytest.mark.parametrize("c", wp.OUT_CONV_CASES, ids=_ids(wp.OUT_CONV_CASES))
def test_taps_behind_a_convolution_axis(c):
    """M = 256, 1024, 2048 and 4096 against 144 lines, on both axes"""
    _check(c)
    px, py, planned = wp.grid_plan(c.nx, c.ny)
    assert planned and {px.kind, py.kind} & {"conv", "conv2k", "conv4k"} and {l[0] for l in _layouts(c)} == {"x", "y"}


@pytest.mark.parametrize("c", wp.OUT_GENERIC_CASES, ids=_ids(wp.OUT_GENERIC_CASES))
def test_taps_behind_the_generic_one_pass_kernel(c):
    _check(c)
    px, py, planned = wp.grid_plan(c.nx, c.ny)
    assert planned and "generic" in (px.kind, py.kind)


@pytest.mark.parametrize("c", wp.OUT_TWO_PASS_CASES, ids=_ids(wp.OUT_TWO_PASS_CASES))
def test_taps_of_the_two_pass_loop(c):
    """slice_loop (fft_path = 1): the row launch leaves (P_y / ny) fft_y psi_k, the gather applies ny conj(P_y)"""
    _check(c)
    assert all(l == ("two-pass", "natural", 0, "generic", "generic") for l in _layouts(c))


@pytest.mark.parametrize("nx,ny,nz", wp.OUT_TDS_LOOP_CASES, ids=["x".join(map(str, g)) for g in wp.OUT_TDS_LOOP_CASES])
def test_taps_of_the_tds_two_pass_loop(nx, ny, nz):
    """slice_loop with the split row step of the handle while msl_set_tds is on.  The stack is built from atoms under absorption (the
    loop needs its weights), the float64 reference runs on the device's own transmission, the probes are white"""
    res = wp.tds_loop_case(nx, ny, nz)
    tol = wp.two_pass_tolerance(nx, ny)
    above = []
    for k, m in sorted(res["taps"].items()):
        above += _within(f"tap after slice {k}", m, wp.bounds(nx, ny, nz, True, layer=k, tol=tol))
    above += _within("exit", res["exit"], wp.bounds(nx, ny, nz, True, tol=tol))
    assert sorted(res["taps"]) == list(range(nz - 1))
    assert res["tds_loop"], "the byte count is not that of the split row step"
    assert res["t_range"] > 0.1, "the built stack is (nearly) vacuum"
    assert not above, above


@pytest.mark.parametrize("c", wp.OUT_PROBE_CHUNK_CASES, ids=_ids(wp.OUT_PROBE_CHUNK_CASES))
def test_taps_past_one_and_two_chunks_of_probes(c):
    _check(c)


@pytest.mark.parametrize("c", wp.OUT_WINDOW_BIN_CASES, ids=_ids(wp.OUT_WINDOW_BIN_CASES))
def test_window_and_bin_on_taps_and_exit(c):
    """the k-window on the fast column kernel (wy % 32 = 0) and on the generic pass, the bin alone and behind a window, the generic
    epilogue and the two-pass loop"""
    _check(c)
    want_column = {(256, 256, (64, 96)): "fast", (256, 256, (50, 40)): "generic", (256, 256, None): "fast", (1024, 256, (256, 64)): "fast",
                   (600, 135, (150, 45)): "generic", (45, 63, (15, 21)): "generic"}[(c.nx, c.ny, c.window)]
    assert all(l[4] == want_column for l in _layouts(c))


@pytest.mark.parametrize("c", wp.OUT_FRAME_BATCH_CASES, ids=_ids(wp.OUT_FRAME_BATCH_CASES))
def test_two_batch_slots_through_the_taps(c):
    """out_group on the fast column kernel and on the generic pass, bin_frames regrouping the staged images by frame: every block of
    slot 0 is more than 1 away from the reference of slot 1 (two independent white fields: sqrt 2)"""
    res = _check(c)
    assert "cross" in res and all(l[4] == ("fast" if c.nx == 256 else "generic") for l in _layouts(c))


def test_wide_download_is_the_complex64_blocks_widened():
    """layers_c128(): (P, T, wx, wy, L) complex128 equals the (L, P, T, wx, wy) complex64 blocks, bit for bit; on white input no
    pixel is (nearly) zero, so every pixel counts"""
    res = _check(wp.OUT_WIDE_CASE, wide=True)
    assert res["wide_equal"] and res["wide_nonzero"] == 1.0
