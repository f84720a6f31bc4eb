"""White-spectrum parity of the slice-loop pass kernels, per image, per line and per pixel (tools/white_parity.py).

The physical-input tests put nearly all of their energy inside a quarter of Nyquist and inside a probe a few angstrom wide, and
bound one energy-weighted norm: an error of several per cent on the outer nine tenths of k-space, or on the lines far from the
probe, passes them.  Here the probes are white noise and every slice is a unit-modulus random phase screen, so every output of
every pass carries the same weight, and besides the image norm (E_img) every single row and column (E_line) and every pixel
(E_pix) is bounded, against the float64 oracle.

Bounds: the white-noise contract of test_fft2_matches_numpy per 2-D transform -- 3e-6 with both axes on a direct kernel, 1e-5
with an axis on a padded convolution (two transforms of >= 2n) -- added in quadrature over the n_t = 2 (nz - 1) transforms of the
loop (one more for the fused spectrum; one tolerance for a single-slice exit wave, which has none): E_img <= tol sqrt(n_t),
E_line <= 2 tol sqrt(n_t) (a line is a smaller sample of the same homogeneous error), E_pix <= 10 tol sqrt(n_t) (the largest of
~1e5 Rayleigh-distributed errors is about 3.4 rms; a complex64 CPU evaluation of the loop shows 4.1 - 4.7).  A complex64
torch.fft run of the loop gives E_img 2.2e-7 - 4.9e-7, E_line <= 7.3e-7, E_pix <= 1.9e-6 on these inputs.
Run on the MI355X box with `pytest -m gpu`; `python tools/white_parity.py profiles/white_spectrum_parity.txt` records the measured
figures per kernel family (a record: the bounds are not taken from it).
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def _check(nx, ny, nz, P=2):
    res = wp.white_case(nx, ny, nz, P)
    assert res["one_pass"], "the slice loop did not run its one-pass kernels on this grid"
    for name in ("exit", "spectrum"):
        lim = wp.bounds(nx, ny, nz, name == "spectrum")
        print(f"{nx} x {ny} x {nz} P={P} {name}: E_img {res[name][0]:.3e} E_line {res[name][1]:.3e} E_pix {res[name][2]:.3e}"
              f" (bounds {lim[0]:.2e} {lim[1]:.2e} {lim[2]:.2e})")
    for name in ("exit", "spectrum"):
        lim = wp.bounds(nx, ny, nz, name == "spectrum")
        for what, v, b in zip(("E_img", "E_line", "E_pix"), res[name], lim):
            assert v <= b, f"{name} {what} {v:.3e} above {b:.3e}"


def test_the_length_list_is_every_direct_length():
    from pyslice_amd import _native
    assert wp.DIRECT_LENGTHS == _native.fast_lengths(129, 2048)
    assert len(wp.DIRECT_LENGTHS) == 103 and len(wp.MIXED_LENGTHS) == 99
    assert all(_native.line_kernel_class(n) == 1 for n in wp.MIXED_LENGTHS)
    assert all(_native.line_kernel_class(n) == 2 for n in wp.POW2_LENGTHS)
    assert _native.line_kernel_class(135) == 1 and _native.line_kernel_class(144) == 1      # the direct cross axes
    assert all(_native.line_kernel_class(n) == 0 for n in wp.CONV_LENGTHS if n != 192) and _native.line_kernel_class(37) == 0
    assert {c[0] for c in wp.MIXED_CASES if c[1] == 135 and c[2] == 3} == set(wp.MIXED_LENGTHS)
    assert {c[1] for c in wp.MIXED_CASES if c[0] == 135 and c[2] == 2} == set(wp.MIXED_LENGTHS)
    assert {n for c in wp.POW2_CASES for n in c[:2]} >= set(wp.POW2_LENGTHS)


@pytest.mark.parametrize("nx,ny,nz", wp.MIXED_CASES, ids=_ids(wp.MIXED_CASES))
def test_every_mixed_radix_length_on_both_axes(nx, ny, nz):
    """each of the 99 rowTM / rowTM2 instantiations along x (nz = 3) and along y (nz = 2), 135 lines: a partial last tile"""
    _check(nx, ny, nz)


@pytest.mark.parametrize("nx,ny,nz", wp.POW2_CASES, ids=_ids(wp.POW2_CASES))
def test_power_of_two_kernels(nx, ny, nz):
    """rowT / row2 (256, 1024), the 2R^2 kernel (512), the 2048-point wave kernel: against a mixed-radix and a convolution cross
    axis, and paired with each other (alternating scheme, interleaved and paired work-buffer layouts)"""
    _check(nx, ny, nz)


@pytest.mark.parametrize("nx,ny,nz", wp.CONV_CASES, ids=_ids(wp.CONV_CASES))
def test_convolution_and_generic_lengths_at_their_edges(nx, ny, nz):
    """rowTB / rowTB2 / rowTC2 at the smallest and largest length of every cyclic length M, where the wrapped lags of the filter
    reach the line ends, and the generic one-pass kernel"""
    _check(nx, ny, nz)


@pytest.mark.parametrize("nx,ny,nz,P", wp.MANY_PROBE_CASES, ids=_ids(wp.MANY_PROBE_CASES))
def test_probe_chunks_with_white_input(nx, ny, nz, P):
    """one and two chunks of 16 probes plus one: every probe is checked (the metrics take the worst image)"""
    _check(nx, ny, nz, P)


def test_frame_batch_slots_get_their_own_white_potential():
    nx, ny, nz = wp.FRAME_BATCH_CASE
    m0, m1, cross = wp.frame_batch_case(nx, ny, nz)
    lim = wp.bounds(nx, ny, nz, True)
    print(f"frame 0 {m0}, frame 1 {m1}, bounds {lim}, frame 0 against the reference of frame 1: {cross:.3f}")
    for m in (m0, m1):
        for v, b in zip(m, lim):
            assert v <= b
    assert cross > 1.0          # two independent white fields: rel-L2 about sqrt(2)


@pytest.mark.parametrize("nx,ny,nz", wp.SINGLE_SLICE_CASES, ids=_ids(wp.SINGLE_SLICE_CASES))
def test_single_slice_is_transmission_times_probe(nx, ny, nz):
    """nz = 1: no propagation, the exit wave is t psi and the spectrum its fft2"""
    probes, V = wp.white_input(nx, ny, 1, 2)
    want, _ = wp.reference(probes, V[0], nx, ny, 1)
    t = np.exp(1j * wp.orc.interaction_sigma(wp.EV) * V[0, 0].astype(np.float64))
    assert rel_l2(want, t[None] * probes) < 1e-14          # the reference of a single slice is the plain product
    _check(nx, ny, 1)
