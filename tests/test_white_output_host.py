"""Host checks of output_case(), tap_layout() and the OUT_* lists of tools/white_parity.py, the yardstick of
tests/test_gpu_white_output.py: no device needed.

- the untilted reference with layers= is the oracle's loop on the truncated stack, and stored() is the crop-then-block-sum definition;
- a complex64 evaluation of the loop, cropped and binned in float32, stays inside the bounds for every window / bin case of the
  lists: a window is a crop of a homogeneous error field and a coherent block sum adds error and signal alike in quadrature, so the
  white-noise contract holds unchanged for the stored form;
- tap_layout() is tied to the lines of mslice.hip it restates, and the lists together reach every gather order, both rp, every
  conj(P) site, both column passes (each with window, bin and frame scatter) and both two-pass loops;
- each fault a tap or the output stage can have, applied to the float64 reference rounded to complex64, exceeds its bound in the
  metric named (the ratios are printed);
- the call order and the block / slot indexing of output_case on a float64 engine.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import rel_l2
from test_white_tilt_host import Float64Engine, axis_table

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)
orc = wp.orc

SRC = open(os.path.join(os.path.dirname(__file__), "..", "pyslice_amd", "csrc", "mslice.hip")).read()
ALL_CASES = [(name, c) for name, cases in wp.OUTPUT_LISTS for c in cases]
STORED_CASES = [c for c in wp.OUT_WINDOW_BIN_CASES + wp.OUT_FRAME_BATCH_CASES if c.window or c.k_bin]


@pytest.fixture(autouse=True)
def pure_tolerance(monkeypatch):
    """wp.tolerance without the library call: a direct kernel on both axes (a mixed-radix or power-of-two length) or not"""
    direct = lambda n: n in wp.POW2_LENGTHS or n in wp._mixed_groups()
    monkeypatch.setattr(wp, "tolerance", lambda nx, ny: wp.TOL_DIRECT if direct(nx) and direct(ny) else wp.TOL_CONV)


def test_untilted_layer_reference_is_the_oracle_on_the_truncated_stack():
    nx, ny, nz = 45, 63, 4
    probes, V = wp.white_input(nx, ny, nz, 2)
    ex, spec, taps = wp.reference(probes, V[0], nx, ny, nz, layers=(0, 1, 2))
    xs, ys = np.arange(nx) * wp.DX, np.arange(ny) * wp.DY
    for k in range(nz):
        want = orc.diffraction(orc.propagate(probes, np.moveaxis(V[0, :k + 1].astype(np.float64), 0, 2), xs, ys, np.arange(k + 1) * wp.DZ, wp.EV))
        assert rel_l2(taps[k] if k < nz - 1 else spec, want) < 1e-13, k


@pytest.mark.parametrize("nx,ny,window,k_bin", [(45, 63, (15, 21), (5, 7)), (64, 48, None, (4, 2)), (64, 48, (50, 40), None), (33, 20, (9, 8), (3, 4))])
def test_stored_is_crop_then_block_sum(nx, ny, window, k_bin):
    rng = np.random.default_rng(nx)
    full = rng.standard_normal((2, 3, nx, ny)) + 1j * rng.standard_normal((2, 3, nx, ny))
    got = wp.stored(full, nx, ny, window, k_bin)
    wx, wy = window or (nx, ny)
    bx, by = k_bin or (1, 1)
    x0, y0 = nx // 2 - wx // 2, ny // 2 - wy // 2
    assert got.shape == (2, 3, wx // bx, wy // by)
    # the definition of test_k_bin_is_a_block_sum_of_the_full_spectrum, and pixel by pixel
    win = full[:, :, x0:x0 + wx, y0:y0 + wy]
    assert np.array_equal(got, win.reshape(2, 3, wx // bx, bx, wy // by, by).sum(axis=(3, 5)))
    for i in range(wx // bx):
        for j in range(wy // by):
            want = sum(full[:, :, x0 + i * bx + a, y0 + j * by + b] for a in range(bx) for b in range(by))
            assert np.abs(got[:, :, i, j] - want).max() < 1e-12
    assert np.array_equal(wp.stored(full, nx, ny), full)


def c64_blocks(probes, V, layers):
    """the loop in complex64 (float32 FFTs): the spectra of the taps and of the exit, fftshifted, complex64"""
    import torch
    psi = torch.from_numpy(probes.astype(np.complex64))
    nz, nx, ny = V.shape
    prop = torch.from_numpy((axis_table(nx, wp.DX, 0.0)[:, None] * axis_table(ny, wp.DY, 0.0)[None, :]).astype(np.complex64))
    sig = np.float32(orc.interaction_sigma(wp.EV))
    out = {}
    for z in range(nz):
        ph = torch.from_numpy(V[z]) * sig
        psi = torch.complex(torch.cos(ph), torch.sin(ph)) * psi
        if z in layers or z == nz - 1:
            out[z] = torch.fft.fftshift(torch.fft.fft2(psi), dim=(-2, -1))
        if z < nz - 1:
            psi = torch.fft.ifft2(prop * torch.fft.fft2(psi))
    assert all(v.dtype == torch.complex64 for v in out.values())
    return out


@pytest.mark.parametrize("c", STORED_CASES, ids=[wp.output_id(c) for c in STORED_CASES])
def test_complex64_loop_cropped_and_binned_in_float32_is_inside_the_bounds(c):
    """section 2 of the contract: the bounds of the full spectra hold for the stored form"""
    import torch
    probes, V, want = wp.output_data(c.nx, c.ny, c.nz, c.P, c.layers, c.frame_batch)
    wx, wy = c.window or (c.nx, c.ny)
    bx, by = c.k_bin or (1, 1)
    x0, y0 = c.nx // 2 - wx // 2, c.ny // 2 - wy // 2
    for b in range(c.frame_batch):
        got = c64_blocks(probes, V[b], c.layers)
        for k, g in got.items():
            s = g[:, x0:x0 + wx, y0:y0 + wy].reshape(c.P, wx // bx, bx, wy // by, by).sum(dim=(2, 4))
            assert s.dtype == torch.complex64
            full = want[b][0] if k == c.nz - 1 else want[b][1][k]
            m, lim = wp.metrics(s.numpy(), wp.stored(full, c.nx, c.ny, c.window, c.k_bin)), wp.case_bounds(c, None if k == c.nz - 1 else k)
            print(f"{wp.output_id(c)} slot {b} block {k}: " + " ".join(f"{v:.2e}" for v in m) + " of bounds " + " ".join(f"{v / l:.2f}" for v, l in zip(m, lim)))
            assert all(v <= l for v, l in zip(m, lim)), (k, m, lim)


def test_tap_layout_restates_the_loops_the_tap_order_and_fast_ok():
    # the lines restated
    for line in ("return h->scheme_b ? ((s & 1) != 0) : (((h->cfg.nz - 1 - s) & 1) != 0);",
                 "h->scheme_b = h->onepass && !(h->opx.kind == AX_FOURSTEP && h->opy.kind == AX_FOURSTEP);",
                 "flags |= (k > 0 ? P2_IN_PAIRED : 0) | (k < nz - 2 ? P2_OUT_PAIRED : 0);",
                 "j.perm_shift = ((along_y ? h->Rx : h->Ry) == 32) ? 2 : 1;",
                 "const int order = (j.flags & P2_OUT_PAIRED) ? TAP_INTERLEAVED : TAP_NATURAL;",
                 "tap_step(h, k, fused_slot, groups, along_y ? h->psiT : h->psi, along_y, order, 8 << j.perm_shift, along_y ? 0 : 1)",
                 "if (h->opx.kind == AX_WAVE2K && h->opy.kind == AX_WAVE2K)",
                 "if (interleaves(h->opx) && interleaves(h->opy) && !dbg_env(\"MSL_NO_INTERLEAVE\") && h->debug_flags_mask < 0) {",
                 "j.perm_shift = (((k & 1) ? h->opy : h->opx).R == 32) ? 2 : 1;",
                 "tap_step(h, k, fused_slot, groups, (k & 1) ? h->psi : h->psiT, !(k & 1), order, rp, (k & 1) ? 1 : 0)",
                 "bool interleaves(const msl_handle::OpDir& o) { return o.kind == AX_FOURSTEP || o.kind == AX_TWO; }",
                 "if (!(flags & P2_OUT_PAIRED)) return TAP_NATURAL;",
                 "if (o.kind == AX_WAVE2K) return TAP_PAIRED;",
                 "return interleaves(o) ? TAP_INTERLEAVED : TAP_NATURAL;",
                 "const bool fast_ok = h->Rx && c.ny % 32 == 0 && (!windowed || h->wy % 32 == 0);",
                 "if (ry && cfg->nx % (256 / ry) == 0) { h->Ry = ry;",
                 "if (rx && cfg->ny % 16 == 0 && cfg->ny >= 32) { h->Rx = rx;",
                 "int fast_radix(int n) { return n == 1024 ? 32 : (n == 256 ? 16 : 0); }",
                 "tap_step(h, z, fused_slot, groups, h->psi, false, TAP_NATURAL, 8, 2)",
                 "} else if ((n == 512 || n == 2048) && lines_ok && !dbg_env(\"MSL_NO_TWO\")) {",
                 "} else if (n >= 33 && n <= 512 && (n <= 128 || n >= 192 || plan_M != n) && !dbg_env(\"MSL_NO_BLUESTEIN_REG\")) {",
                 "} else if (n >= 513 && n <= 1024 && !dbg_env(\"MSL_NO_BLUESTEIN_REG\")) {",
                 "} else if (n >= 1025 && n <= 2047 && !dbg_env(\"MSL_NO_CONV4096\") && !dbg_env(\"MSL_NO_BLUESTEIN_REG\")) {",
                 "} else if (plan_M <= 1024 && !dbg_env(\"MSL_NO_GENERIC_ONEPASS\")) {",
                 "if ((rc = begin_timed(h, (sums ? 5 : 2) * nz + 2 + (fused ? tap_launches(h) : 0)))) return rc;",
                 "if ((z > 0 && (rc = row_step(z, true, false))) || (rc = slice_sums_hook(h, P, z)) || (rc = row_step(z, false, true))) return rc;",
                 "if ((timed && (rc = timer.begin(h))) || (rc = slice_loop(h, slot, groups, first_group, h->tds_on || h->ion_on))) return rc;",
                 "if ((rc = transpose_probes(h)) || (rc = slice_loop(h, -1, 1, h->cur_batch))) return rc;"):
        assert line in SRC, line
    # alternating scheme: interleaved up to k = nz - 3 in the order of the READING kernel, natural at nz - 2, at both parities
    assert [wp.tap_layout(256, 256, 4, k) for k in range(3)] == [("x", "interleaved", 16, "fast", "fast"), ("y", "interleaved", 16, "fast", "fast"),
                                                                 ("x", "natural", 0, "fast", "fast")]
    assert [wp.tap_layout(256, 256, 5, k)[:2] for k in range(4)] == [("y", "interleaved"), ("x", "interleaved"), ("y", "interleaved"), ("x", "natural")]
    assert [wp.tap_layout(1024, 256, 4, k)[:3] for k in range(3)] == [("x", "interleaved", 16), ("y", "interleaved", 32), ("x", "natural", 0)]
    assert [wp.tap_layout(256, 1024, 4, k)[:3] for k in range(3)] == [("x", "interleaved", 32), ("y", "interleaved", 16), ("x", "natural", 0)]
    # scheme B: even passes along y; a pass along y is read by the kernel of x
    assert [wp.tap_layout(1024, 512, 4, k)[:3] for k in range(3)] == [("y", "interleaved", 32), ("x", "interleaved", 16), ("y", "interleaved", 32)]
    assert [wp.tap_layout(512, 256, 4, k) for k in range(2)] == [("y", "interleaved", 16, "fast", "generic"), ("x", "interleaved", 16, "fast", "generic")]
    assert [wp.tap_layout(2048, 2048, 4, k)[:3] for k in range(3)] == [("y", "paired", 0), ("x", "paired", 0), ("y", "paired", 0)]
    assert wp.tap_layout(2048, 512, 4, 0)[:3] == ("y", "natural", 0) and wp.tap_layout(2048, 144, 4, 1)[:3] == ("x", "natural", 0)
    # fast_ok: ny % 32 = 16 and a window with wy % 32 != 0 take the generic column pass, Rx needs 16 | ny and ny >= 32
    assert wp.tap_layout(256, 144, 4, 1)[3:] == ("generic", "generic") and wp.tap_layout(256, 160, 4, 1)[4] == "fast"
    assert wp.tap_layout(256, 256, 4, 0, window=(64, 96))[4] == "fast" and wp.tap_layout(256, 256, 4, 0, window=(50, 40))[4] == "generic"
    assert wp.tap_layout(256, 256, 4, 0, window=(50, 64))[4] == "fast" and wp.tap_layout(256, 256, 4, 0, window=(256, 256))[4] == "fast"
    assert wp.plan_radices(256, 16) == (0, 0) and wp.plan_radices(136, 1024) == (0, 32) and wp.plan_radices(132, 1024) == (0, 0)
    assert wp.plan_radices(256, 256, fft_path=1) == (0, 0)
    assert wp.tap_layout(45, 63, 4, 1, one_pass=False, fft_path=1) == ("two-pass", "natural", 0, "generic", "generic")
    assert wp.tap_layout(2048, 144, 4, 1, one_pass=False)[0] == "two-pass"          # (a tilt fallback: fft_path = 0 on the two-pass loop)
    # the plan of an axis: the families of family(), named as plan_axis_kind names them
    kinds = {n: wp.axis_plan(n, 144, wp.plan_radices(n, 144)[0]) for n in (127, 501, 997, 1025, 143, 32, 600, 1000, 512, 2048, 256)}
    assert [kinds[n].kind for n in (127, 501, 997, 1025, 143, 32, 600, 1000, 512, 2048, 256)] == \
        ["conv", "conv", "conv2k", "conv4k", "generic", "generic", "mixed", "mixed", "two", "wave2k", "fourstep"]
    assert (kinds[127].R, kinds[501].R, kinds[512].R, kinds[256].R, wp.axis_plan(1024, 144, 32).R) == (16, 32, 16, 16, 32)
    assert wp.axis_plan(512, 135, 0).kind == "conv" and wp.axis_plan(2048, 135, 0).base is None and wp.axis_plan(2049, 144, 0).base is None
    assert wp.grid_plan(45, 63, fft_path=1)[2] is False and wp.grid_plan(501, 144)[2] is True


def test_every_listed_case_has_the_layout_of_its_list():
    for name, c in ALL_CASES:
        px, py, planned = wp.grid_plan(c.nx, c.ny, c.fft_path)
        assert planned == (not c.fft_path), (name, c)
        for k in c.layers:
            lay = wp.tap_layout(c.nx, c.ny, c.nz, k, planned, c.window, c.fft_path)
            assert lay[0] == wp.tap_axis(c.nx, c.ny, c.nz, k, planned), (name, c, k)
        # the stored shape divides into bins, and the window lies inside the grid
        wx, wy = c.window or (c.nx, c.ny)
        bx, by = c.k_bin or (1, 1)
        assert wx <= c.nx and wy <= c.ny and wx % bx == 0 and wy % by == 0 and c.layers == tuple(range(c.nz - 1))
    assert [tuple(c[:2]) for c in wp.OUT_UNTILTED_CASES] == [tuple(c[:2]) for c in wp.TILT_LAYER_CASES]
    orders = lambda cases: {wp.tap_layout(c.nx, c.ny, c.nz, k, True, c.window)[1] for c in cases for k in c.layers}
    assert orders(wp.OUT_PAIRED_CASES) == {"paired"} and orders(wp.OUT_SCHEME_B_CASES) == {"interleaved"}
    assert orders(wp.OUT_WAVE_NATURAL_CASES) == orders(wp.OUT_ROWTM2_CASES) == orders(wp.OUT_CONV_CASES) == orders(wp.OUT_GENERIC_CASES) == {"natural"}
    for c in wp.OUT_ALTERNATING_CASES[:3]:
        assert [wp.tap_layout(c.nx, c.ny, c.nz, k)[1] for k in c.layers] == ["interleaved"] * (c.nz - 2) + ["natural"]
    for c in wp.OUT_SCHEME_B_CASES:
        px, py, _ = wp.grid_plan(c.nx, c.ny)
        assert {px.kind, py.kind} == {"two", "fourstep"}                            # 512 against 256 (equal R') and 1024 (unequal)
    assert {(wp.grid_plan(c.nx, c.ny)[0].R, wp.grid_plan(c.nx, c.ny)[1].R) for c in wp.OUT_SCHEME_B_CASES} == {(16, 16), (32, 16), (16, 32)}
    assert all(wp.family(*wp.axis_under_test(c.nx, c.ny)) == "wave-2K" for c in wp.OUT_WAVE_NATURAL_CASES)
    assert all(wp._mixed_groups()[1000] == 64 and 1000 in (c.nx, c.ny) for c in wp.OUT_ROWTM2_CASES)
    assert wp._mixed_groups()[wp.OUT_MIXED16_CASES[0].nx] == 16
    M = {"conv": lambda n: 256 if n <= 128 else 1024, "conv2k": lambda n: 2048, "conv4k": lambda n: 4096}
    for axis in (0, 1):
        got = set()
        for c in wp.OUT_CONV_CASES:
            p = wp.grid_plan(c.nx, c.ny)[axis]
            if p.kind in M:
                got.add(M[p.kind]((c.nx, c.ny)[axis]))
        assert got == {256, 1024, 2048, 4096}, axis
    assert all("generic" in (wp.grid_plan(c.nx, c.ny)[0].kind, wp.grid_plan(c.nx, c.ny)[1].kind) for c in wp.OUT_GENERIC_CASES)
    assert [c.P for c in wp.OUT_PROBE_CHUNK_CASES] == [17, 33]


def test_the_lists_together_reach_every_path():
    """the assertion that keeps a later edit of the lists from emptying a path"""
    seen, stage = set(), set()
    for name, c in ALL_CASES:
        planned = wp.grid_plan(c.nx, c.ny, c.fft_path)[2]
        for k in c.layers:
            axis, order, rp, row, col = wp.tap_layout(c.nx, c.ny, c.nz, k, planned, c.window, c.fft_path)
            seen |= {("order", order), ("rp", rp), ("row", axis, row), ("column", axis, col), ("loop", axis == "two-pass")}
            if axis != "two-pass" and wp.grid_plan(c.nx, c.ny)[0].kind == wp.grid_plan(c.nx, c.ny)[1].kind == "fourstep":
                seen.add(("alternating parity", c.nz & 1, order))
            stage |= {(col, what) for what, on in (("window", c.window), ("bin", c.k_bin), ("frame scatter", c.frame_batch > 1)) if on}
    assert {("order", o) for o in ("natural", "interleaved", "paired")} <= seen
    assert {("rp", 16), ("rp", 32)} <= seen
    assert {("row", "y", "fast"), ("row", "y", "generic")} <= seen                  # conj(P_y) in the fast and in the generic row FFT
    assert {("column", "x", "fast"), ("column", "x", "generic")} <= seen            # conj(P_x): COL_MULPX, and MUL_VEC of the generic pass
    assert {("alternating parity", p, o) for p in (0, 1) for o in ("interleaved", "natural")} <= seen
    assert {("loop", True), ("loop", False)} <= seen and len(wp.OUT_TDS_LOOP_CASES) >= 1      # both forms of the two-pass loop: the plain row step and the split one
    assert {(col, what) for col in ("fast", "generic") for what in ("window", "bin", "frame scatter")} <= stage
    # the untilted grids include the tap behind a convolution axis, the two-pass window / bin case is there, and a frame batch is binned
    assert wp.grid_plan(501, 144)[0].kind == "conv" and any((c.nx, c.ny) == (501, 144) for c in wp.OUT_UNTILTED_CASES)
    assert any(c.fft_path and c.window and c.k_bin for c in wp.OUT_WINDOW_BIN_CASES)
    assert any(c.frame_batch == 2 and c.window and c.k_bin for c in wp.OUT_FRAME_BATCH_CASES)


def test_loop_bytes_is_the_count_of_the_library():
    assert "h->ctr.algorithmic_bytes += (uint64_t)P * c.nz * bytes * npix + (uint64_t)groups * c.nz * 8ull * npix + (fused ? (uint64_t)P * 16ull * npix : 0ull);" in SRC
    assert "h->ctr.algorithmic_bytes += (uint64_t)P * (img * (axis == 2 ? 3 : 5) + (uint64_t)h->wpix * 8ull);" in SRC
    assert "count_slice_loop(h, P, groups, fused, 32 + 16 + 8);" in SRC and "h->ctr.algorithmic_bytes += (uint64_t)nz * h->tds_n * 4ull * npix;" in SRC
    # without taps and one frame: the count white_case checks, plus the fused spectrum
    assert wp.loop_bytes(600, 135, 3, 2, 1, 0, 600 * 135, True) == (16 * 2 + 8) * 3 * 600 * 135 + 2 * 16 * 600 * 135
    assert wp.loop_bytes(45, 63, 4, 2, 2, 3, 9, False) == 4 * 4 * 32 * 2835 + 2 * 4 * 8 * 2835 + 4 * 16 * 2835 + 3 * 4 * (2835 * 24 + 72)
    assert wp.tds_loop_bytes(45, 63, 4, 2, 3, 2835) == 2 * 4 * 56 * 2835 + 4 * 8 * 2835 + 2 * 16 * 2835 + 4 * 4 * 2835 + 3 * 2 * (2835 * 24 + 2835 * 8)


# ---- detection -------------------------------------------------------------------------------------------------------------------
def _shifted_table(n, d):
    return np.fft.fftshift(axis_table(n, d, 0.0))


def test_each_fault_of_a_tap_or_of_the_output_stage_exceeds_its_bound():
    nx, ny, nz, P, layers = 256, 256, 4, 2, (0, 1, 2)
    probes, V, want = wp.output_data(nx, ny, nz, P, layers, 2)
    k = 1                                                       # the tap after slice 1 of 256 x 256 x 4: pass along y, interleaved, rp 16
    axis, order, rp = wp.tap_layout(nx, ny, nz, k)[:3]
    assert (axis, order, rp) == ("y", "interleaved", 16)
    full = want[0][1][k]
    lim = wp.bounds(nx, ny, nz, True, layer=k)
    assert lim[0] == 3e-6 * np.sqrt(3)
    c64 = lambda a: np.asarray(a).astype(np.complex64)
    clean = wp.metrics(c64(full), full)
    print("unfaulted, rounded to complex64: " + " ".join(f"{v:.2e}" for v in clean))
    assert clean[0] < 2e-7 and clean[1] < 2e-7 and all(v < b / 10 for v, b in zip(clean, lim))
    Px, Py = _shifted_table(nx, wp.DX)[:, None], _shifted_table(ny, wp.DY)[None, :]
    # S = A_y psi_k as the pass left it, in real space (P, nx, ny), and its spectrum with conj(P_y): the tap's own arithmetic
    S = np.fft.ifft2(np.fft.ifftshift(full * Py, axes=(1, 2)))
    tap = lambda s: np.conj(Py) * np.fft.fftshift(np.fft.fft2(s), axes=(1, 2))
    assert wp.metrics(tap(S), full)[0] < 1e-13
    faults = {}
    faults["conj(P_d) dropped at a tap"] = ("E_img", full * Py, full, lim)
    faults["conjugate of the other axis applied"] = ("E_img", full * Py * np.conj(Px), full, lim)
    # the work buffer holds the lines along x (the reading kernel's), position 2 R' (j >> 1) + 2 l + (j & 1) = element R' j + l
    s = S.copy()
    pos = np.arange(2 * rp)
    s[0, :2 * rp, 5] = S[0, rp * (pos & 1) + (pos >> 1), 5]     # one block of 2 rp of one line read as natural
    faults["interleaved block of 2 rp read as natural"] = ("E_line", tap(s), full, lim)
    s = S.copy()
    s[0, :, 6], s[0, :, 7] = S[0, :, 7], S[0, :, 6]
    faults["the two lines of a pair swapped"] = ("E_line", tap(s), full, lim)
    g = full.copy()
    g[:, 1:, 48:56], g[:, 0, 48:56] = full[:, :-1, 48:56], 0.0
    faults["8 columns of a 16-column tile moved to the next row"] = ("E_line", g, full, lim)
    window, k_bin = (64, 96), (4, 4)
    st = wp.stored(full, nx, ny, window)
    x0, y0 = nx // 2 - 32, ny // 2 - 48
    faults["window origin off by one pixel"] = ("E_img", full[:, x0 + 1:x0 + 65, y0:y0 + 96], st, lim)
    faults["window origin off by one 16-column tile"] = ("E_img", full[:, x0:x0 + 64, y0 + 16:y0 + 112], st, lim)
    binned = wp.stored(full, nx, ny, None, k_bin)
    g = binned.copy()
    g[1, 9, 33] -= full[1, 9 * 4 + 2, 33 * 4 + 1]
    faults["one binned pixel short of one addend"] = ("E_pix", g, binned, lim)
    g = full.copy()
    i = np.unravel_index(np.argsort(np.abs(full[0]).ravel())[full[0].size // 2], full[0].shape)      # a pixel of median modulus
    g[(0,) + i] *= 1.0 + 1e-3
    faults["one pixel off by 1e-3 of its value"] = ("E_pix", g, full, lim)
    for name, (metric, got, ref, b) in faults.items():
        i = ("E_img", "E_line", "E_pix").index(metric)
        m = wp.metrics(c64(got), ref)
        print(f"{name}: {metric} {m[i]:.3e}, {m[i] / b[i]:.3g} x the bound {b[i]:.2e}")
        assert m[i] > b[i], name
    # the same faults on the tilted tables' blind spot: without a tilt the conjugate of the other axis is still a fault (P_x != P_y
    # pixel by pixel), which is what the untilted cases add to TILT_LAYER_CASES
    cross_ok = wp._rel_l2(c64(full), want[1][1][k])
    cross_bad = wp._rel_l2(c64(want[1][1][k]), want[1][1][k])
    print(f"taps of batch slot 1 stored in slot 0: cross {cross_bad:.3e} (two independent white fields: {cross_ok:.3f})")
    assert cross_ok > 1.0 and cross_bad < 1.0


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
class OutputEngine(Float64Engine):
    """Float64Engine with the calls output_case() adds: a k-window, a bin, two batch slots and the fused byte count"""

    def __init__(self, nx, ny, nz, P, n_frames=1, fft_path=0, frame_batch=1, window=None, k_bin=None, fault=None):
        super().__init__(nx, ny, nz, P)
        self.n_frames, self.frame_batch, self.window, self.k_bin, self.fft_path = n_frames, frame_batch, window, k_bin, fft_path
        self.fault2, self.slot, self.Vs = fault, 0, {}

    def select_batch_slot(self, b):
        self.calls.append(f"select {b}")
        self.slot = b

    def upload_potential(self, V):
        self.Vs[self.slot] = V

    def set_layers(self, layers):
        self.calls.append("set_layers")
        super().set_layers(layers)

    def _frames(self, first, slots):
        nx, ny, nz = self.shape
        L = len(self.layers) + 1
        wx, wy = wp.stored(np.zeros((1, nx, ny)), nx, ny, self.window, self.k_bin).shape[1:]
        if not hasattr(self, "result"):
            self.result = np.zeros((L, self.P, self.n_frames, wx, wy), dtype=np.complex128)
        for f, b in enumerate(slots):
            self.V = self.Vs[b]
            for l, k in enumerate(self.layers + [nz - 1]):
                src = self.Vs[1] if self.fault2 == "slot 1 in slot 0" and b == 0 and l < L - 1 else self.Vs[b]
                self.V = src
                spec = orc.diffraction(self._loop(k + 1))
                if self.fault2 == "window one tile off" and self.window:
                    spec = np.roll(spec, -16, axis=2)
                self.result[l, :, first + f] = wp.stored(spec, nx, ny, self.window, self.k_bin)
        self.bytes += wp.loop_bytes(nx, ny, nz, self.P, len(slots), len(self.layers), wx * wy, not self.fft_path)
        self.bytes += 8 * nx * ny if self.fault2 == "a launch more" else 0

    def propagate_frame(self, slot):
        self.calls.append("propagate_frame")
        self._frames(slot, [self.slot])

    def propagate_frames(self, first, count):
        self.calls.append(f"propagate_frames {first} {count}")
        self._frames(first, list(range(count)))

    def layers_c64(self):
        self.calls.append("layers_c64")
        return self.result.astype(np.complex64)

    def wavefunction(self):
        self.calls.append("wavefunction")
        return self.result[-1].astype(np.complex64)

    def layers_c128(self):
        return np.moveaxis(self.result.astype(np.complex64), 0, -1).astype(np.complex128)


def test_output_case_plumbing_on_a_float64_engine(monkeypatch):
    made = []

    def fake(fault=None):
        def make(nx, ny, nz, P, **kw):
            made.append(OutputEngine(nx, ny, nz, P, fault=fault, **kw))
            return made[-1]
        return make
    monkeypatch.setattr(wp, "engine", fake())
    nx, ny, nz, layers = 48, 45, 4, (0, 1, 2)
    res = wp.output_case(nx, ny, nz, 2, layers, wide=True)
    assert made[-1].calls == ["set_layers", "propagate_frame", "layers_c64", "wavefunction", "close"]
    assert res["one_pass"] is True and res["exit_is_last_block"] and res["wide_equal"] and "cross" not in res
    assert sorted(res["taps"]) == [(0, 0), (0, 1), (0, 2)] and sorted(res["exit"]) == [0]
    assert max(m[0] for m in list(res["taps"].values()) + [res["exit"][0]]) < 2e-7
    # a window, a bin and two slots: every block of every slot against its own reference, slot 0 far from slot 1's
    res = wp.output_case(nx, ny, nz, 2, layers, window=(32, 15), k_bin=(4, 5), frame_batch=2)
    assert made[-1].calls == ["select 0", "select 1", "set_layers", "propagate_frames 0 2", "layers_c64", "wavefunction", "close"]
    assert (made[-1].window, made[-1].k_bin, made[-1].n_frames, made[-1].frame_batch) == ((32, 15), (4, 5), 2, 2)
    assert sorted(res["taps"]) == [(b, k) for b in (0, 1) for k in layers] and sorted(res["exit"]) == [0, 1]
    assert max(m[0] for m in list(res["taps"].values()) + list(res["exit"].values())) < 2e-7 and res["one_pass"] is True
    assert sorted(res["cross"], key=str) == [0, 1, 2, "exit"] and min(res["cross"].values()) > 1.0
    # the two-pass byte count, and a count that is neither
    assert wp.output_case(nx, ny, nz, 2, layers, fft_path=1)["one_pass"] is False
    monkeypatch.setattr(wp, "engine", fake("a launch more"))
    assert wp.output_case(nx, ny, nz, 2, layers)["one_pass"] is None
    # the taps of slot 1 in slot 0: slot 0's taps are wrong and equal slot 1's reference, its exit and all of slot 1 are right
    monkeypatch.setattr(wp, "engine", fake("slot 1 in slot 0"))
    res = wp.output_case(nx, ny, nz, 2, layers, frame_batch=2)
    assert all(res["taps"][(0, k)][0] > 1.0 and res["cross"][k] < 1e-6 and res["taps"][(1, k)][0] < 2e-7 for k in layers)
    assert res["exit"][0][0] < 2e-7 and res["cross"]["exit"] > 1.0
    # a window one tile off along y: every block above its bound, the unwindowed run untouched
    monkeypatch.setattr(wp, "engine", fake("window one tile off"))
    res = wp.output_case(64, 64, nz, 2, layers, window=(32, 32))
    assert min(m[0] for m in list(res["taps"].values()) + [res["exit"][0]]) > 1.0
    assert wp.output_case(64, 64, nz, 2, layers)["exit"][0][0] < 2e-7
